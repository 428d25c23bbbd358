// Output files of the command-line tools (`zkeynew`, `ptauprepare`, `zkeycontribute`): written under a temporary name, <path>.partial,
// renamed by commit() and removed otherwise, so that a failure leaves neither <path> nor <path>.partial behind.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
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

// A container (binfile: magic, version, section table) rewritten from another one through a mapping: some sections copied,
// the others left for libzkhip to fill in place.  The constructor refuses an output that is the input; write() lays the
// file out; commit() renames it.
struct ContainerOut {
    struct Section {
        uint32_t id;
        uint64_t size;
        const uint8_t *src;                                // copied from here; null: the payload is left to the caller
    };
    std::string path;
    std::unique_ptr<MappedOutFile> file;
    ContainerOut(const std::string &inPath, const std::string &outPath) : path(outPath) {
        struct stat a, b;
        if (stat(inPath.c_str(), &a) == 0 && stat(outPath.c_str(), &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)
            throw std::invalid_argument("the input and the output are the same file");
    }
    // -> where each section's payload starts in the mapping, in the order of `secs`
    std::vector<uint8_t *> write(const uint8_t magicVersion[8], const std::vector<Section> &secs) {
        uint64_t total = 12;
        for (const auto &s : secs) total += 12 + s.size;
        file.reset(new MappedOutFile(path, total));
        uint8_t *at = file->data;
        const uint32_t count = (uint32_t)secs.size();
        memcpy(at, magicVersion, 8);
        memcpy(at + 8, &count, 4);
        at += 12;
        std::vector<uint8_t *> payload;
        for (const auto &s : secs) {
            memcpy(at, &s.id, 4);
            memcpy(at + 4, &s.size, 8);
            at += 12;
            payload.push_back(at);
            if (s.src) memcpy(at, s.src, s.size);
            at += s.size;
        }
        return payload;
    }
    void commit() { file->commit(); }
};
