// The long rows of a coefficient CSR (fieldops.hip): what launch_csr_build counted, and the
// descriptors the sums over them need.  One per CSR: a prover's, or an operator call's.
#pragma once
#include "hiputil.hpp"
#include "kernels.hpp"

namespace zkp {

struct CsrLong {
    uint32_t cut = 0, long_rows = 0, chunks = 0, longest = 0;
    DevBuf<uint4> long_desc, chunk_desc;
    DevBuf<uint32_t> counters;      // two words the descriptor kernels count in (kept with the descriptors: no wait at build)
    // stats: the four words of launch_csr_build's err, on the host (the caller has waited for them anyway).  Nothing is
    // launched or allocated for a CSR without a long row.
    void build(const uint32_t *rowptr, uint32_t rows, uint32_t row_cut, const uint32_t stats[4], hipStream_t s) {
        cut = row_cut;
        long_rows = stats[1];
        chunks = stats[2];
        longest = stats[3];
        if (!chunks) return;
        counters.alloc(2);
        long_desc.alloc(long_rows);
        chunk_desc.alloc(chunks);
        zk::launch_csr_long_rows(long_desc.p, chunk_desc.p, counters.p, rowptr, rows, cut, long_rows, chunks, s);
    }
    zk::CsrDev view(const uint32_t *rowptr, const uint32_t *col, const zk::Fr *val) const {
        zk::CsrDev c{rowptr, col, val};
        if (chunks) {
            c.chunk_desc = chunk_desc.p;
            c.long_desc = long_desc.p;
            c.chunks = chunks;
            c.long_rows = long_rows;
            c.cut = cut;
        }
        return c;
    }
};

}   // namespace zkp
