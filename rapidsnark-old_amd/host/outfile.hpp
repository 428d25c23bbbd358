// Output files of the command-line tools (`zkeynew`, `ptauprepare`): written under a temporary name, <path>.partial,
// renamed by commit() and removed otherwise, so that a failure leaves neither <path> nor <path>.partial behind.
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

// a file written through a stream
struct OutFile {
    std::string path, tmp;
    std::ofstream f;
    bool done = false;
    explicit OutFile(const std::string &p) : path(p), tmp(p + ".partial") {
        f.open(tmp, std::ios::binary | std::ios::trunc);
        if (!f) throw std::runtime_error("cannot write " + path);
    }
    void write(const void *p, uint64_t n) { f.write(static_cast<const char *>(p), (std::streamsize)n); }
    void u32(uint32_t v) { write(&v, 4); }
    void section(uint32_t id, uint64_t size) {
        u32(id);
        write(&size, 8);
    }
    void commit() {
        f.close();
        if (!f) throw std::runtime_error("cannot write " + path);
        if (rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot write " + path);
        done = true;
    }
    ~OutFile() {
        if (!done) {
            f.close();
            remove(tmp.c_str());
        }
    }
};

// a file of a size known in advance, written through a mapping (libzkhip fills sections of it in place)
struct MappedOutFile {
    std::string path, tmp;
    uint8_t *data = nullptr;
    uint64_t size = 0;
    bool done = false;
    MappedOutFile(const std::string &p, uint64_t bytes) : path(p), tmp(p + ".partial"), size(bytes) {
        const int fd = open(tmp.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) throw std::runtime_error("cannot write " + path);
        void *m = ftruncate(fd, (off_t)bytes) == 0 ? mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
        close(fd);
        if (m == MAP_FAILED) {
            remove(tmp.c_str());
            throw std::runtime_error("cannot write " + path);
        }
        data = static_cast<uint8_t *>(m);
    }
    MappedOutFile(const MappedOutFile &) = delete;
    MappedOutFile &operator=(const MappedOutFile &) = delete;
    void commit() {
        const bool ok = msync(data, size, MS_SYNC) == 0;
        munmap(data, size);
        data = nullptr;
        if (!ok || rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot write " + path);
        done = true;
    }
    ~MappedOutFile() {
        if (data) munmap(data, size);
        if (!done) remove(tmp.c_str());
    }
};
