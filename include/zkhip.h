/* zkhip.h — C ABI of the MI355X-native Groth16 hot path (libzkhip.so).
 *
 * The reference (iden3/rapidsnark-old) has no FFI layer: its seam is the C++ template
 * `Groth16::Prover<Engine>` (reference src/groth16.hpp:37-121).  This header is the
 * C-ABI a maintainer would bind in its place; every entry point cites the reference
 * interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Byte conventions are the reference's own:
 *   Fr / Fq element : 32 bytes little-endian (== FrElement / 4 x u64)
 *   G1 affine       : x|y, Montgomery form (R = 2^256), 64 bytes; all-zero = infinity
 *   G2 affine       : x.a|x.b|y.a|y.b, Montgomery form, 128 bytes
 *   witness         : nVars x 32 B, standard (non-Montgomery) form   (src/main_prover.cpp:74)
 *
 * All functions return 0 on success, non-zero on error; zk_last_error() gives the
 * message for the calling thread.  Nothing throws across this boundary.  There is NO
 * CPU fallback: if no HIP device is usable every call fails with an error.
 */
#ifndef ZKHIP_H
#define ZKHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_prover zk_prover;

/* The 15 arguments of Groth16::makeProver<Engine>() (src/groth16.hpp:104-121,
 * call site src/main_prover.cpp:57-73), plus section byte sizes for bounds checks. */
typedef struct zk_zkey_view {
    uint32_t nVars;
    uint32_t nPublic;
    uint32_t domainSize;
    uint64_t nCoefs;
    const void *vk_alpha1;   /* G1, zkey section 2 */
    const void *vk_beta1;    /* G1 */
    const void *vk_beta2;    /* G2 */
    const void *vk_delta1;   /* G1 */
    const void *vk_delta2;   /* G2 */
    const void *coefs;       /* section 4 INCLUDING its leading u32 count (src/groth16.cpp:38 skips 4 bytes) */
    const void *pointsA;     /* section 5: nVars x G1 */
    const void *pointsB1;    /* section 6: nVars x G1 */
    const void *pointsB2;    /* section 7: nVars x G2 */
    const void *pointsC;     /* section 8: (nVars-nPublic-1) x G1 */
    const void *pointsH;     /* section 9: domainSize x G1 */
    uint64_t coefs_bytes, pointsA_bytes, pointsB1_bytes, pointsB2_bytes, pointsC_bytes, pointsH_bytes;
} zk_zkey_view;

typedef struct zk_opts {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    uint32_t shard_index;    /* this prover holds shard `shard_index` of `shard_count` of every MSM   */
    uint32_t shard_count;    /*   point table (contiguous index slices); 0 or 1 = whole    */
    uint32_t window_bits;    /* Pippenger window c; 0 = choose from the size                           */
    uint32_t flags;          /* ZK_FLAG_* */
    uint32_t batch;          /* 0/1 = one witness per submission; 2..ZK_MAX_BATCH = up to that many witnesses of this
                              * circuit proved by ONE set of kernel launches (zk_prove_batch_*; small circuits, where a
                              * proof is bound by kernel latencies: DESIGN.md section 5).  Needs ZK_FLAG_PRECOMP, unsharded. */
} zk_opts;
#define ZK_MAX_BATCH 16

#define ZK_FLAG_TIMINGS 1u   /* record per-stage hipEvent timings (zk_prover_timings) */
#define ZK_FLAG_PARTITIONED_CHAIN 4u   /* sharded provers only (shard_count 2, 4 or 8): the A.w/B.w rows and the six
                              * transforms are PARTITIONED over the shards too (each holds the block of rows its H
                              * table slice covers) instead of replicated; such provers are driven through
                              * zk_multi_prove* (one process) or zk_shard_* (one process per GPU) */
#define ZK_FLAG_PRECOMP 2u   /* window-precomputed point tables: W x the table memory in HBM and a longer
                              * zk_prover_create, ~19 % fewer point additions per proof (same results) */

#define ZK_FLAG_PRECOMP_HALF 16u   /* (implies ZK_FLAG_PRECOMP) table rows for every SECOND window only: ceil(W/2) x the table memory
                              * instead of W x (7 instead of 13 at c = 20) and the same additions per point.  The digits of the odd
                              * windows add the neighbouring even window's row into a second bucket set, whose sum the host doubles
                              * c times: two bucket reductions per MSM instead of one.  For provers that hold several keys
                              * (proverServer, src/main_proofserver.cpp:12-26) and for circuits whose full tables do not fit (2^25
                              * on one MI355X).  Same proofs.  Not with opts.batch. */
#define ZK_FLAG_SPARSE_WITNESS 8u   /* with ZK_FLAG_PRECOMP: the four witness MSMs (A, B1, B2, C; src/groth16.cpp:180-204) use a
                              * 16-bit window (2^15 buckets per set) instead of the size-based one (2^19 at 2^22 constraints).
                              * For CIRCUIT witnesses — mostly 0, 1 and small values: few non-zero digits — the additions are few
                              * and the bucket reductions, which do not shrink with the witness, dominate those MSMs; with
                              * uniformly random scalars (the benchmark's worst case) it costs three more additions per point.
                              * Same proofs either way.  MSM H (scalars a.b - c: always full-size) keeps its window. */

/* Same bytes as Proof<Engine>{A,B,C} (src/groth16.hpp:13-24): affine, Montgomery LE. */
typedef struct zk_proof {
    uint8_t A[64];
    uint8_t B[128];
    uint8_t C[64];
} zk_proof;

/* The five multi-exponentiation results of src/groth16.cpp:171-204 before the final
 * assembly, as affine Montgomery points (all-zero = infinity).  With sharding these are
 * PARTIAL sums over this prover's slice; partial sums add up across shards. */
typedef struct zk_msm_sums {
    uint8_t pih[64];
    uint8_t pi_a[64];
    uint8_t pib1[64];
    uint8_t pi_b[128];
    uint8_t pi_c[64];
} zk_msm_sums;

const char *zk_last_error(void);
int zk_device_count(int *count);

/* makeProver (src/groth16.cpp:9-46) + Prover ctor (src/groth16.hpp:57-95).  One-off work:
 * CSR build of the coefficient records, upload of the point tables and twiddle tables.
 * The host image may be freed after this returns (the reference Prover borrows it). */
int zk_prover_create(zk_prover **out, const zk_zkey_view *zkey, const zk_opts *opts);
void zk_prover_destroy(zk_prover *p);

/* Prover::prove (src/groth16.cpp:48-254).  wtns: nVars x 32 B standard form (host memory).
 * r32/s32: 32-byte LE scalars replacing randombytes_buf (src/groth16.cpp:216-217); NULL
 * draws 31 random bytes each exactly as the reference does. */
int zk_prove(zk_prover *p, const uint8_t *wtns, const uint8_t *r32, const uint8_t *s32, zk_proof *out);
/* Same with the witness already resident in device memory (HBM) on the prover's device. */
int zk_prove_dev(zk_prover *p, const void *d_wtns, const uint8_t *r32, const uint8_t *s32, zk_proof *out);

/* Throughput mode: the same prove(), split so that consecutive proofs overlap.  The reference
 * proves strictly one at a time (src/fullprover.cpp:96-97: one worker thread); on the GPU the
 * latency-bound front of proof k+1 (digit sort, A.w/B.w, NTTs) hides under the tail of proof k
 * (bucket reductions, D2H, host Horner + final assembly, src/groth16.cpp:219-251).
 * zk_prove_dev_submit enqueues all device work of one proof and returns; at most ZK_MAX_IN_FLIGHT
 * proofs may be in flight per prover; per-proof buffers are allocated the first time a depth is reached.
 * Large circuits: two keep the chip busy when witnesses are resident in HBM, a third and fourth hide the upload of a
 * host witness (a proof cannot start before its witness has arrived).  Small circuits (below ~2^19) are
 * bound by the serial latency of their ~60 small kernels, not by throughput: there more proofs in flight
 * (on the prover's four lanes of streams) and batched submissions are what fills the GPU.  zk_prove_collect blocks until the OLDEST submitted proof is complete
 * and writes it.  d_wtns must stay valid (and unmodified) until its proof has been collected;
 * r32/s32 are copied at submit (NULL = random, drawn at collect).  On a sharded prover the pair is
 * zk_prove_dev_submit (r32/s32 ignored) + zk_prove_msm_collect, which hands back this shard's
 * partial sums for zk_prove_finish. */
#define ZK_MAX_IN_FLIGHT 8
int zk_prove_dev_submit(zk_prover *p, const void *d_wtns, const uint8_t *r32, const uint8_t *s32);
/* The same with the witness in HOST memory — the reference's own contract, Prover::prove(FrElement
 * *wtns) (src/groth16.hpp:101, call sites src/main_prover.cpp:74-75, src/fullprover.cpp:155).  The
 * upload runs on a stream of its own into a per-proof HBM buffer, so the witness of proof k+1 goes
 * up while proof k computes, and the call itself returns at once: a pageable buffer is copied to
 * pinned staging by a host function on that stream, a buffer from zk_host_alloc (or otherwise
 * page-locked) is read by the DMA engine directly.  Either way `wtns` must stay valid and untouched
 * until its proof has been collected (as for zk_prove_dev_submit). */
int zk_prove_submit(zk_prover *p, const uint8_t *wtns, const uint8_t *r32, const uint8_t *s32);
/* Page-locked host memory for witnesses (what a witness generator or a .wtns reader should fill:
 * src/fullprover.cpp:139-145 reads the file into a malloc'ed image, src/binfile_utils.cpp:28-33). */
int zk_host_alloc(void **out, size_t bytes);
void zk_host_free(void *ptr);
int zk_prove_collect(zk_prover *p, zk_proof *out);
/* Per-proof workspace is allocated the first time a slot / lane is used (the one-shot CLI never needs more than one).  A
 * server that will keep `in_flight` proofs in flight calls this once after create: every proof slot and lane such a
 * pipeline walks (in_flight + 1 slots of the ring, at most ZK_MAX_IN_FLIGHT; slot 0 alone for 1) is allocated NOW — with
 * host_witnesses != 0 including the per-slot HBM witness buffer and its pinned staging copy — so that running out of
 * device memory is a start-up error the caller can react to (tables as in the zkey instead of the window-precomputed
 * ones) and never a failed proof later.  Replaces nothing in the reference (its workspace is `new FrElement[]` per proof,
 * src/groth16.cpp:52-60). */
int zk_prover_reserve(zk_prover *p, uint32_t in_flight, uint32_t host_witnesses);
/* What zk_prover_create decided for this key on this device — the launch plan a benchmark, a server or a log line reports
 * (and sizes its pipeline by) instead of re-deriving the library's rules.  Set plan->size = sizeof(zk_prover_plan) before
 * the call (fields may be appended in later versions; only `size` bytes are written).  Replaces nothing in the
 * reference: its plan is fixed in code (one proof at a time, src/fullprover.cpp:96-97; window chosen inside ffiasm). */
typedef struct zk_prover_plan {
    uint32_t size;
    uint32_t window_bits_h, windows_h;     /* Pippenger window c of MSM H; digits = point additions per point */
    uint32_t window_bits_w, windows_w;     /* the same for the witness MSMs A, B1, B2, C (differs with ZK_FLAG_SPARSE_WITNESS) */
    uint32_t precomputed_tables;           /* 0: tables as in the zkey; 1: ZK_FLAG_PRECOMP (a row per window); 2: ZK_FLAG_PRECOMP_HALF (a row per second window) */
    uint32_t msm_a_b1_c_one_launch;        /* MSM A, B1, C as ONE set of launches over three tables (blockIdx.y) */
    uint32_t lanes;                        /* independent sets of compute streams: proof k runs on lane k % lanes */
    uint32_t follow_up_streams;            /* high-priority streams for merges / reductions (sharded provers) */
    uint32_t max_in_flight;                /* ZK_MAX_IN_FLIGHT */
    uint32_t depth_host_witness;           /* proofs in flight that saturate this prover: witnesses in host memory ... */
    uint32_t depth_resident_witness;       /* ... and already resident in HBM (no upload to hide) */
    uint32_t batch;                        /* opts.batch in effect (1 = single-witness submissions) */
    uint32_t shard_index, shard_count, chain_partitioned;
    uint64_t device_bytes_in_use;          /* HBM in use on the prover's device right now (all processes), from the runtime */
    uint64_t device_bytes_total;
    uint64_t kernel_launches_last_proof;   /* kernel launches the most recently submitted proof took (0 before the first; a graph replay counts as none) */
    uint32_t table_rows_h, table_rows_w;   /* rows of n points per table (x the zkey's table memory): windows_* with ZK_FLAG_PRECOMP, ceil(windows_* / 2) with _HALF, else 1 */
    uint32_t bucket_sets_h, bucket_sets_w; /* bucket sets (= bucket reductions) per MSM: 1 with ZK_FLAG_PRECOMP, 2 with _HALF, windows_* with plain tables */
    /* A.w / B.w (src/groth16.cpp:62-85): rows of more than spmv_row_cut terms are summed chunk by chunk, a wave each, instead
     * of by the row's one lane.  A sharded prover counts the rows it computes. */
    uint32_t spmv_row_cut;                 /* the cut in effect (ZKHIP_SPMV_ROW_CUT at create, else the built-in one; 0: no row is long) */
    uint32_t spmv_long_rows;               /* local rows of A and B above it */
    uint32_t spmv_longest_row;             /* terms of the longest local row */
    uint32_t spmv_chunks;                  /* chunks of up to 1024 terms the long rows make; 0 = the lane-per-row kernel alone */
} zk_prover_plan;
int zk_prover_info(zk_prover *p, zk_prover_plan *plan);
int zk_prove_msm_collect(zk_prover *p, zk_msm_sums *partial);
/* Batched proving (a prover created with opts.batch = B >= 2): `count` (1..B) witnesses of the circuit, given as
 * `count` host pointers, are proved by ONE submission — one digit sort with a bucket set per witness, one set of
 * accumulation / merge / reduction launches over all of them, the A.w/B.w rows and the transforms batched — which is
 * what a server for Semaphore-class circuits wants: there a proof is a chain of ~60 latency-bound kernels, and four
 * proofs in one chain cost little more than one.  The reference has no counterpart (one
 * Prover::prove per request, src/fullprover.cpp:154-159); every proof is the one zk_prove would give for the same
 * (witness, r, s).  r32s / s32s: count x 32 bytes or NULL (drawn at collect).  A submission occupies one of the
 * ZK_MAX_IN_FLIGHT slots; zk_prove_batch_collect takes the OLDEST submission, which must carry `count` proofs.  The
 * single-witness entry points work on a batch prover too (a submission of one). */
int zk_prove_batch_submit(zk_prover *p, const uint8_t *const *wtns, uint32_t count, const uint8_t *r32s, const uint8_t *s32s);
int zk_prove_batch_collect(zk_prover *p, zk_proof *out, uint32_t count);

/* Multi-GPU split of prove(): steps 1-10 (src/groth16.cpp:52-204) on this prover's shard ... */
int zk_prove_msm_dev(zk_prover *p, const void *d_wtns, zk_msm_sums *partial);
int zk_prove_msm(zk_prover *p, const uint8_t *wtns, zk_msm_sums *partial);
/* ... and steps 11-13 (src/groth16.cpp:209-253) over the partial sums of all shards (host, O(1)). */
int zk_prove_finish(zk_prover *p, const zk_msm_sums *partials, uint32_t n_partials,
                    const uint8_t *r32, const uint8_t *s32, zk_proof *out);

/* ---- one proof on several GPUs with the chain PARTITIONED too (north_star: "the five MSMs and the NTT
 * partitioned across the 8 GPUs").  GPU g holds rows [g*n/G, (g+1)*n/G) of a = A.w, b = B.w, c, h (the
 * slice its H table covers), runs the stages over the low log2(n/G) index bits of the six transforms
 * (src/groth16.cpp:98-155) locally and meets the others only in the log2(G) top stages: one radix-G
 * butterfly per block offset, for which each GPU receives 1/G of every block (all-to-all), computes,
 * and returns the results (all-to-all) — 2 x (G-1)/G of a block per GPU and transform over xGMI.
 *
 * (a) All GPUs in ONE process — what the reference's CLI / server are (src/main_prover.cpp:57-75,
 *     src/fullprover.cpp:154-159).  One shard prover per device inside; blocks exchanged by peer
 *     writes, cross-device ordering by events; one host thread enqueues everything.  devices may name
 *     the same device several times (all shards on one GPU: how the tests exercise this path on a
 *     1-GPU box).  The chain is partitioned when n_devices is 2, 4 or 8 and domainSize >= n_devices^2
 *     (ZKHIP_REPLICATED_CHAIN=1 in the environment keeps it replicated), otherwise replicated.
 *     zk_multi_prove = Prover::prove; submit/collect as zk_prove_submit / zk_prove_collect. */
typedef struct zk_multi_prover zk_multi_prover;
int zk_multi_prover_create(zk_multi_prover **out, const zk_zkey_view *zkey, const int32_t *devices, uint32_t n_devices,
                           const zk_opts *opts /* device, shard_* ignored */);
void zk_multi_prover_destroy(zk_multi_prover *mp);
int zk_multi_prove(zk_multi_prover *mp, const uint8_t *wtns, const uint8_t *r32, const uint8_t *s32, zk_proof *out);
int zk_multi_prove_submit(zk_multi_prover *mp, const uint8_t *wtns, const uint8_t *r32, const uint8_t *s32);
int zk_multi_prove_collect(zk_multi_prover *mp, zk_proof *out);
int zk_multi_prover_info(zk_multi_prover *mp, uint32_t *n_shards, uint32_t *chain_partitioned);
/* zk_prover_info of shard `shard` (< n_shards): with a partitioned chain every shard holds its own block of rows, so the
 * spmv_* fields differ from shard to shard. */
int zk_multi_prover_shard_info(zk_multi_prover *mp, uint32_t shard, zk_prover_plan *plan);
/* (b) One process per GPU (torch.distributed over RCCL): a prover created with shard_index/shard_count and
 *     ZK_FLAG_PARTITIONED_CHAIN is driven step by step, and the CALLER moves the blocks between the steps
 *     with FOUR all_to_all_single per proof on two buffers it owns and registers here (3 polynomials x
 *     block_elems x 32 bytes each, both laid out [GPU][polynomial][chunk]: `send` is what the library packs
 *     for / unpacks from the collective, `recv` is what the cross stages work on in place):
 *         zk_shard_begin                       rows of a, b, c; packed -> send     all_to_all_single(recv <- send)
 *         zk_shard_step(ZK_STEP_CROSS_INVERSE) top stages in place in recv         all_to_all_single(send <- recv)
 *         zk_shard_step(ZK_STEP_LOCAL)         unpack, local stages + coset, pack  all_to_all_single(recv <- send)
 *         zk_shard_step(ZK_STEP_CROSS_FORWARD) top stages in place in recv         all_to_all_single(send <- recv)
 *         zk_shard_step(ZK_STEP_FINISH)        unpack, h, MSM H, MSM C, joins      zk_prove_msm_collect + zk_prove_finish
 *     `stream` (hipStream_t; NULL = the default stream) is the stream the caller's collectives are ordered
 *     on: every call first waits for what is enqueued on it and makes it wait for what the call enqueued. */
enum { ZK_STEP_CROSS_INVERSE = 1, ZK_STEP_LOCAL = 2, ZK_STEP_CROSS_FORWARD = 3, ZK_STEP_FINISH = 4 };
int zk_shard_info(zk_prover *p, uint64_t *block_elems, uint32_t *chain_partitioned);
int zk_shard_set_exchange(zk_prover *p, void *d_send, void *d_recv);
int zk_shard_begin(zk_prover *p, const uint8_t *wtns, const void *d_wtns, const uint8_t *r32, const uint8_t *s32, void *stream);
int zk_shard_step(zk_prover *p, int step, void *stream);

/* Same as zk_prove_finish without a prover object: pure host code, usable on a rank that owns
 * no GPU (e.g. a coordinator).  vk points as in zk_zkey_view. */
int zk_assemble(const void *vk_alpha1, const void *vk_beta1, const void *vk_beta2, const void *vk_delta1,
                const void *vk_delta2, const zk_msm_sums *partials, uint32_t n_partials,
                const uint8_t *r32, const uint8_t *s32, zk_proof *out);

/* Device times of the last prove, ms (needs ZK_FLAG_TIMINGS), from hipEvents on the library's own
 * streams.  Two streams overlap (h chain | witness MSMs), so stage walls are not additive;
 * ZK_T_G1_L1_KERNEL is the mean duration of the four launches of the G1 level-1 accumulation kernel of the
 * last proof (MSM A, B1, C, H; events immediately before/after each launch, on its stream), ZK_T_G2_L1_KERNEL
 * the one launch of the G2 kernel, ZK_T_WTNS_H2D the witness upload of a host-witness proof. */
enum {
    ZK_T_SPMV = 0, ZK_T_NTT, ZK_T_DIGITS_SORT, ZK_T_MSM_H, ZK_T_JOIN_WAIT, ZK_T_MSM_REDUCE,
    ZK_T_TOTAL_DEVICE, ZK_T_G1_L1_KERNEL, ZK_T_G2_L1_KERNEL, ZK_T_WTNS_H2D, ZK_T_COUNT
};
int zk_prover_timings(zk_prover *p, double *ms, uint32_t n);

/* ---- operator-level entry points (host pointers; staged through the device) ------------- */
/* out[i] = a[i]*b[i]*R^-1 mod r  — E.fr.mul (src/groth16.cpp:91-95). */
int zk_fr_mul_vec(uint8_t *out, const uint8_t *a, const uint8_t *b, uint64_t n);
/* same over Fq — E.f1.mul */
int zk_fq_mul_vec(uint8_t *out, const uint8_t *a, const uint8_t *b, uint64_t n);
/* a = A.w, b = B.w: the coefficient accumulation of src/groth16.cpp:62-85 as an operator.  coefs = zkey
 * section 4 INCLUDING its leading u32 count (packed 44-byte records, src/groth16.hpp:27-35); wtns standard
 * form; a, b (domainSize x 32 B each) come back in the reference's Montgomery form. */
int zk_fr_coef_accumulate(uint8_t *a, uint8_t *b, const void *coefs, uint64_t nCoefs, uint32_t domainSize,
                          const uint8_t *wtns, uint32_t nVars);
/* In-place natural-order NTT over Fr, Montgomery in/out: inverse=0 -> FFT::fft, 1 -> FFT::ifft
 * (incl. 1/n) (src/groth16.cpp:102,115).  n must be a power of two <= 2^28. */
int zk_fr_ntt(uint8_t *data, uint64_t n, int inverse);
/* The whole a/b/c pipeline of src/groth16.cpp:88-163 on host vectors a,b (Montgomery, n each):
 * h[i] = fromMontgomery(A(w2n^(2i+1))*B(..) - C(..)), standard form. */
int zk_fr_abc_to_h(uint8_t *h, const uint8_t *a, const uint8_t *b, uint64_t n);
/* out = sum scalars[i]*bases[i] — Curve::multiMulByScalar (src/groth16.cpp:173,197) with
 * scalarSize = 32; result as AFFINE Montgomery (all-zero = infinity). */
int zk_msm_g1(uint8_t out[64], const uint8_t *bases, const uint8_t *scalars, uint64_t n);
int zk_msm_g2(uint8_t out[128], const uint8_t *bases, const uint8_t *scalars, uint64_t n);
/* The first step of every MSM, shown: the signed-digit recoding and the bucket sort of a scalar vector, as zk_msm_g1/g2
 * (table_mode 0, window_bits 0) and the prover (its table mode and window) run it.  Set plan->size = sizeof(zk_msm_sort_plan)
 * before the call (only `size` bytes are written).  With offsets == NULL and entries == NULL only the plan is filled: no
 * device is touched, so this works on a machine without a GPU.  Otherwise the scalars (`batch` vectors of n each, back to
 * back, 32 B LE standard form; values >= r are reduced first) are uploaded and sorted, and offsets[0 .. total_buckets] and
 * entries[0 .. E) come back, E = offsets[total_buckets] = plan->entries <= max_entries.  batch: 0 or 1 = one vector.
 *
 * What the arrays mean.  A scalar k < r is written k = sum_w d_w 2^(c w), w < W, with signed digits
 * -2^(c-1) <= d_w < 2^(c-1) (a window value >= 2^(c-1) becomes negative and carries into the next window; the top digit is
 * never negative).  Every NON-ZERO digit of every scalar is one entry, and the entries of bucket b are
 * entries[offsets[b] .. offsets[b+1]), in no particular order inside a bucket.  The bucket gives |d| and the bucket set:
 * b = set * nbuckets + (|d| - 1), nbuckets = 2^(c-1).  An entry word is  row | (d < 0 ? 1u << 31 : 0) : the point the
 * digit's magnitude multiplies is row `row` of the MSM's point table, negated when bit 31 is set.  Per table mode
 * (i = index of the scalar in its vector):
 *   0, tables as in the zkey:       sets = W, set = w;        row = i (the point itself; the host combines the W set sums)
 *   1, a table row per window:      sets = 1, set = 0;        row = w * n + i (the table holds 2^(c w) P_i)
 *      with batch > 1:              sets = batch, set = v, the vector; row = w * n + i as before: vectors share the table
 *   2, a row per second window:     sets = 2, set = w & 1;    row = (w >> 1) * n + i (the table holds 2^(2c u) P_i;
 *                                   the host doubles the sum of set 1 c times)
 * plan->n is the number of scalars sorted (batch * n), max_entries = max(plan->n, 1) * W.
 * Errors: table_mode > 2, batch > 1 with table_mode != 1, n * batch * W >= 2^32 or table rows >= 2^31. */
typedef struct zk_msm_sort_plan {
    uint32_t size, c, W, sets, nbuckets, total_buckets, table_mode, batch;
    uint64_t n, max_entries, entries;
} zk_msm_sort_plan;
int zk_msm_sort(const uint8_t *scalars, uint64_t n, uint32_t window_bits, uint32_t table_mode, uint32_t batch,
                zk_msm_sort_plan *plan, uint32_t *offsets /* total_buckets + 1 */, uint32_t *entries /* max_entries */);

/* ---- synthetic tables & single-point helpers (benchmark inputs) ------ */
/* out[i] = P0 + i*Q, affine Montgomery, generated on the GPU (host output buffer). */
int zk_synth_chain_g1(uint8_t *out, uint64_t n, const uint8_t p0[64], const uint8_t q[64]);
int zk_synth_chain_g2(uint8_t *out, uint64_t n, const uint8_t p0[128], const uint8_t q[128]);
/* Batch fixed-base multiplication out[i] = scalars[i] * base (affine Montgomery out, scalars n x 32 B
 * LE standard form, 0 -> all-zero infinity encoding), on the GPU.  What a Groth16 setup does with the
 * evaluations A_i(tau), B_i(tau), ... (snarkjs zkey sections 5-9 as consumed at src/main_prover.cpp:67-72):
 * with it trapdoor-valid keys at benchmark sizes take seconds. */
int zk_fixed_base_g1(uint8_t *out, const uint8_t base[64], const uint8_t *scalars, uint64_t n);
int zk_fixed_base_g2(uint8_t *out, const uint8_t base[128], const uint8_t *scalars, uint64_t n);
/* out = k*P — Curve::mulByScalar (src/groth16.cpp:223) on the host; k: 32 B LE standard form. */
int zk_g1_mul(uint8_t out[64], const uint8_t p[64], const uint8_t k[32]);
int zk_g2_mul(uint8_t out[128], const uint8_t p[128], const uint8_t k[32]);

/* ---- output formatting (src/groth16.cpp:268-301, src/main_prover.cpp:77-93) - */
/* Compact JSON exactly as nlohmann's operator<< prints Proof::toJson(); returns needed length
 * (excluding NUL); writes at most cap bytes incl. NUL. */
size_t zk_proof_to_json(const zk_proof *proof, char *buf, size_t cap);
/* public.json: ["w1",...,"wN"], or null when nPublic == 0 (reference quirk Q7). */
size_t zk_public_to_json(const uint8_t *wtns, uint32_t nPublic, char *buf, size_t cap);

/* ---- R1CS: check a witness against the circuit's constraints before proving ------------- */
/* Nothing in the reference corresponds to these entry points: Prover::prove (src/groth16.cpp:48-254) trusts its witness
 * and never looks at C, so a witness that breaks a constraint still yields a proof that only the verifier rejects.  The
 * counterpart is snarkjs `wtns check <circuit.r1cs> <witness.wtns>`.  A checker holds circom's .r1cs on one device and
 * runs on a stream of its own (it synchronises that stream only); calls on one checker are serialised.
 * zk_r1cs_view: the .r1cs header and section 2 (constraints) exactly as in the file; the caller has checked the prime
 * (BN254 r).  create range-checks every term: a wire id >= nWires or a coefficient >= r is an error naming the constraint. */
typedef struct zk_r1cs zk_r1cs;
typedef struct zk_r1cs_view {
    uint32_t nWires, nPubOut, nPubIn, nPrvIn, nConstraints;
    const void *constraints;                /* section 2 as in the file */
    uint64_t constraints_bytes;
} zk_r1cs_view;
/* Set rep->size = sizeof(zk_r1cs_report) before a check (as zk_prover_plan: only `size` bytes are written). */
typedef struct zk_r1cs_report {
    uint32_t size;
    uint64_t failed;                        /* constraints with (A.w)(B.w) != C.w */
    uint32_t first_failed;                  /* lowest such constraint; UINT32_MAX: none */
    uint8_t a[32], b[32], c[32];            /* A.w, B.w, C.w of first_failed, standard form LE (zero when none fails) */
    uint32_t one_ok;                        /* w[0] == 1 (the verifier assumes it) */
    uint32_t first_unreduced;               /* lowest index of a witness value >= r; UINT32_MAX: none */
} zk_r1cs_report;
int zk_r1cs_create(zk_r1cs **out, const zk_r1cs_view *v, int32_t device);      /* device -1: the current one */
void zk_r1cs_destroy(zk_r1cs *r);
/* wtns: nVars x 32 B standard form in host memory / in HBM on the checker's device.  nVars != nWires is an error, not a
 * report.  A device witness must be complete when the call is made (the checker's stream does not wait for others). */
int zk_r1cs_check(zk_r1cs *r, const uint8_t *wtns, uint32_t nVars, zk_r1cs_report *rep);
int zk_r1cs_check_dev(zk_r1cs *r, const void *d_wtns, uint32_t nVars, zk_r1cs_report *rep);
/* Was this .zkey made from this circuit?  Sizes first (nVars == nWires, nPublic == nPubOut + nPubIn, domainSize >=
 * nConstraints + nPublic + 1: a mismatch is an error), then A and B as linear maps: A.x and B.x for one random x from
 * the zkey's coefficient records and from the .r1cs, compared row by row — rows below nConstraints equal, zkey row
 * nConstraints + i = (x_i, 0) for i <= nPublic (snarkjs's public-input rows), later rows 0.  A difference goes
 * undetected with probability ~1/r.  C is not in a .zkey, so the match cannot cover it.  first_row: UINT32_MAX = none. */
int zk_r1cs_match_zkey(zk_r1cs *r, const zk_zkey_view *zkey, uint64_t *rows_differing, uint32_t *first_row);

/* ---- Groth16 setup: a .zkey from circom's .r1cs and a prepared Powers of Tau file -------- */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is snarkjs `groth16 setup circuit.r1cs pot.ptau circuit_0000.zkey` (alias `zkey new`): the phase-2 starting
 * key, gamma = delta = 1.  zk_ptau_view: the .ptau's power, alpha1 (section 4 point 0), beta1 (section 5 point 0), beta2
 * (section 6) and the Lagrange-basis sections 12 (tauG1), 13 (tauG2), 14 (alphaTauG1), 15 (betaTauG1) that `powersoftau
 * prepare phase2` writes, as pointers and byte sizes into the mapped file: points as in a .zkey, level p of a section
 * (2^p points) starts at point 2^p - 1; section 12 holds levels 0 .. power + 1, the others 0 .. power.  NULL section
 * pointers: the file is not prepared for phase 2.  Only levels k and k + 1 of section 12 and level k of the others are
 * read (2^k: the circuit's domain), never a whole section. */
typedef struct zk_ptau_view {
    uint32_t power;
    const void *alpha1, *beta1, *beta2;     /* G1, G1, G2 */
    const void *lagrange_g1, *lagrange_g2, *lagrange_alpha_g1, *lagrange_beta_g1;   /* sections 12, 13, 14, 15 */
    uint64_t lagrange_g1_bytes, lagrange_g2_bytes, lagrange_alpha_g1_bytes, lagrange_beta_g1_bytes;
} zk_ptau_view;
/* What the key of this circuit holds: nVars = nWires, nPublic = nPubOut + nPubIn, domainSize = 2^k (the smallest power
 * of two >= nConstraints + nPublic + 1, at least 2), nCoefs = A and B terms of the .r1cs + nPublic + 1 public-input rows. */
typedef struct zk_setup_sizes {
    uint32_t nVars, nPublic, domainSize, log_domain;
    uint64_t nCoefs;
} zk_setup_sizes;
/* Caller buffers of zkey sections 3 to 9, sized from zk_setup_sizes.  Section 4 holds the records in a fixed order: the A
 * terms constraint by constraint (file order within a constraint), then the public-input rows (A, constraint
 * nConstraints + i, wire i, value 1, i = 0 .. nPublic), then the B terms constraint by constraint. */
typedef struct zk_setup_out {
    uint8_t *coefs;          /* section 4: 4 + nCoefs x 44 bytes, its leading u32 count included (values: value * R^2 mod r) */
    uint8_t *pointsIC;       /* section 3: (nPublic + 1) x 64 */
    uint8_t *pointsA;        /* section 5: nVars x 64 */
    uint8_t *pointsB1;       /* section 6: nVars x 64 */
    uint8_t *pointsB2;       /* section 7: nVars x 128 */
    uint8_t *pointsC;        /* section 8: (nVars - nPublic - 1) x 64 */
    uint8_t *pointsH;        /* section 9: domainSize x 64 */
} zk_setup_out;
/* Checks both files against each other without touching a device: the circuit needs 2^k and the .ptau holds 2^power
 * (k > power), k > 27 (the prover's limit), a .ptau not prepared for phase 2, a Lagrange section shorter than its power
 * needs, a .r1cs section that does not walk.  Returns 0 and the sizes, or an error with its message. */
int zk_groth16_setup_sizes(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, zk_setup_sizes *sizes);
/* The key's sections 3 to 9 on `device` (-1: the current one).  Section 2 is the caller's: nVars, nPublic, domainSize,
 * alpha1, beta1, beta2 from the .ptau, gamma2 = delta2 = the G2 generator, delta1 = the G1 generator.  Free HBM is
 * checked before anything is allocated (out of memory is an error, never a half-made key).  Wire ids and coefficients are
 * range-checked as by zk_r1cs_create. */
int zk_groth16_setup(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, int32_t device, zk_setup_out *out);

/* ---- Powers of Tau: prepare phase 2 (the Lagrange sections 12 to 15 of a .ptau) ---------- */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is snarkjs `powersoftau prepare phase2 pot.ptau pot_prepared.ptau`.
 * An operator per group: out = the 2^log_n affine points (1 / n) sum_k w^(-jk) P_k, j < n = 2^log_n, the inverse DFT over
 * group elements of the first n inputs in natural order (w: the n-th root of unity of zk_fr_ntt); inputs at index >=
 * n_points count as infinity.  Points in the .zkey / .ptau encoding (affine Montgomery, all-zero = infinity), log_n <= 28.
 * With P_k = [tau^k] G this is out_j = [L_j^(n)(tau)] G, one level of a Lagrange section.  Every input is checked against
 * the curve equation (the twist's in G2; coordinates below q): a point that is not on the curve is an error that names
 * its index.  Membership of the G2 subgroup is NOT checked (`powersoftau verify` does that).  device -1: the current one. */
int zk_g1_lagrange(uint8_t *out, const uint8_t *points, uint64_t n_points, uint32_t log_n, int32_t device);
int zk_g2_lagrange(uint8_t *out, const uint8_t *points, uint64_t n_points, uint32_t log_n, int32_t device);
/* The whole file.  zk_ptau_powers_view: the .ptau's power and its sections 2 (tauG1, 2^(power+1) - 1 points), 3 (tauG2),
 * 4 (alphaTauG1), 5 (betaTauG1) (2^power points each) as pointers and byte sizes into the mapped file. */
typedef struct zk_ptau_powers_view {
    uint32_t power;
    const void *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1;               /* sections 2, 3, 4, 5 */
    uint64_t tau_g1_bytes, tau_g2_bytes, alpha_tau_g1_bytes, beta_tau_g1_bytes;
} zk_ptau_powers_view;
/* Byte sizes of sections 12 to 15 (levels 0 .. power + 1 of tauG1: (2^(power+2) - 1) x 64; levels 0 .. power of the
 * others) and the HBM the computation holds at its peak (sections are done one after another: the largest one's). */
typedef struct zk_ptau_lagrange_sizes {
    uint64_t lagrange_g1_bytes, lagrange_g2_bytes, lagrange_alpha_g1_bytes, lagrange_beta_g1_bytes;
    uint64_t device_bytes;
} zk_ptau_lagrange_sizes;
typedef struct zk_ptau_lagrange_out {
    uint8_t *lagrange_g1, *lagrange_g2, *lagrange_alpha_g1, *lagrange_beta_g1;   /* sections 12, 13, 14, 15 */
} zk_ptau_lagrange_out;
/* Checks the view without touching a device: a power outside 1 .. 27 (level power + 1 needs a 2^(power+1)-th root of
 * unity and Fr has roots up to 2^28), a missing section, "ptau section N is short: ... bytes, power P needs ...". */
int zk_ptau_prepare_sizes(const zk_ptau_powers_view *ptau, zk_ptau_lagrange_sizes *sizes);
/* Fills the four caller buffers (they may be a mapping of the output file; a section is written in two pieces, its top
 * level and the levels below it, as each is finished).  Free HBM is checked before anything is allocated: too little
 * is an error naming the bytes needed and free.  A point off the curve is an error naming its section and index. */
int zk_ptau_prepare(const zk_ptau_powers_view *ptau, int32_t device, zk_ptau_lagrange_out *out);

/* ---- Phase-2 contribution: delta <- delta d, sections 8 and 9 <- d^-1 (their points) ------ */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is the arithmetic of snarkjs `zkey contribute`.
 * The operator: out[i] = k points[i] for n G1 points (the .zkey encoding: affine Montgomery, all-zero = infinity, which
 * stays all-zero) and ONE scalar k (32 bytes LE, standard form, as zk_g1_mul takes it).  k >= r is an error, k = 0 gives n
 * points at infinity, n = 0 is legal.  Every point is checked (coordinates below q, y^2 = x^3 + 3) before it is used: one
 * that fails is an error naming the lowest such index.  The points go through the device in chunks (ZKHIP_SCALE_CHUNK
 * =<points> in the environment sets their length, 2^20 otherwise) on two buffer sets, so n is not bound by the HBM.
 * ZKHIP_SCALE_PLAIN=1 computes the same bytes by the plain 254-bit double-and-add (the yardstick of the timing tool).
 * device -1: the current one. */
int zk_g1_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t k[32], int32_t device);
/* What the host makes of k before the kernel runs, for a check without a device: k = k1 + k2 lambda by BN254's
 * endomorphism (lambda = 4407920970296243842393367215006156084916469457145843978461, |k1|, |k2| < 2^127), recoded as one
 * joint signed-digit schedule: *len <= ZK_SCALE_PLAN_MAX columns, digits in {-1, 0, 1}, least significant first, with
 *     sum_i 2^i (digits_p[i] + lambda digits_phi[i]) = k  (mod r).
 * cap: the room in both arrays; *len is written even when it exceeds cap (an error).  k >= r is an error. */
#define ZK_SCALE_PLAN_MAX 130
int zk_g1_scale_plan(const uint8_t k[32], int8_t *digits_p, int8_t *digits_phi, uint32_t cap, uint32_t *len);
/* The contribution.  zk_zkey_contrib_view: the key's two delta points (section 2) and its sections 8 (C) and 9 (H) as
 * pointers and byte sizes into the mapped file.  An empty section 8 (every signal public) is legal. */
typedef struct zk_zkey_contrib_view {
    const void *vk_delta1;   /* G1 */
    const void *vk_delta2;   /* G2 */
    const void *pointsC;     /* section 8 */
    const void *pointsH;     /* section 9 */
    uint64_t pointsC_bytes, pointsH_bytes;
} zk_zkey_contrib_view;
typedef struct zk_zkey_contrib_sizes {
    uint64_t pointsC_bytes, pointsH_bytes;   /* of the output sections: those of the input */
    uint64_t chunk_points;                   /* points per chunk in effect */
    uint64_t device_bytes;                   /* HBM the call holds: two buffer sets of one chunk each */
} zk_zkey_contrib_sizes;
typedef struct zk_zkey_contrib_out {
    uint8_t *vk_delta1;      /* 64 bytes */
    uint8_t *vk_delta2;      /* 128 bytes */
    uint8_t *pointsC, *pointsH;
} zk_zkey_contrib_out;
/* Checks the view without touching a device: a section that is not a whole number of points, a delta point that is not on
 * its curve. */
int zk_zkey_contribute_sizes(const zk_zkey_contrib_view *zkey, zk_zkey_contrib_sizes *sizes);
/* vk_delta1 <- d vk_delta1, vk_delta2 <- d vk_delta2 (on the host, the code of zk_g1_mul / zk_g2_mul), every point of
 * sections 8 and 9 <- d^-1 point (zk_g1_scale's kernel, chunk by chunk; the caller buffers may be a mapping of the output
 * file).  d: 32 bytes LE standard form; 0 and d >= r are errors.  Free HBM is checked before anything is allocated: too
 * little is an error naming the bytes needed and free.  A point off the curve is an error naming its section and index.
 * d, d^-1 and everything derived from them are zeroed in host and device memory before the call returns; no message of
 * zk_last_error contains them. */
int zk_zkey_contribute(const zk_zkey_contrib_view *zkey, const uint8_t d[32], int32_t device, zk_zkey_contrib_out *out);

/* ---- Pairing and verification: the optimal ate pairing on BN254, Groth16 verify ---------- */
/* Nothing in the reference corresponds to these entry points (it only proves); the counterpart is snarkjs `groth16
 * verify`.  Points are in the .zkey encoding (affine Montgomery, all-zero = infinity).
 * The pairs (g1[i], g2[i]), i < n_pairs, are taken in consecutive groups of `group` (the last may be shorter); out receives
 * 384 bytes per group: the final-exponentiated product of e(P_i, Q_i) over the group, as 12 Fq values of 32 bytes
 * little-endian in standard form (NOT Montgomery), in the order c0.c0.re, c0.c0.im, c0.c1.re, ... c1.c2.im of
 * Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq2 = Fq[u]/(u^2 + 1), G2 on the D-type twist untwisted by
 * (x, y) -> (x w^2, y w^3).  A pair with a point at infinity contributes 1.  Every point is checked first (coordinates
 * below q, the curve's / the twist's equation, and [r] Q = infinity in G2): one that fails is an error naming its index,
 * "pairing: G2 point 37 is not in the subgroup".  n_pairs = 0 is legal, group = 0 an error.  The groups go through the
 * device in chunks of ZKHIP_VERIFY_CHUNK (2^16 otherwise).  device -1: the current one. */
int zk_pairing(uint8_t *out, const uint8_t *g1, const uint8_t *g2, uint64_t n_pairs, uint32_t group, int32_t device);
/* A verification key on a device.  create checks the key's points (alpha, beta, gamma, delta not infinity and on their
 * curves, the three G2 points in the subgroup, every IC point on the curve), uploads IC, writes the line coefficients of
 * gamma and delta and the Miller value of (alpha, beta) once. */
typedef struct zk_vkey zk_vkey;
typedef struct zk_vkey_view {
    const void *vk_alpha1;                  /* G1, 64 bytes */
    const void *vk_beta2, *vk_gamma2, *vk_delta2;   /* G2, 128 bytes each */
    const void *IC;                         /* (nPublic + 1) x 64 bytes */
    uint32_t nPublic;
} zk_vkey_view;
int zk_vkey_create(zk_vkey **out, const zk_vkey_view *view, int32_t device);
void zk_vkey_destroy(zk_vkey *vk);
/* verdict[i] of proof i: OK; INVALID: well-formed, but e(A, B) != e(alpha, beta) e(vk_x, gamma) e(C, delta); MALFORMED: a
 * coordinate not below q, A or C off the curve, B off the twist or outside the order-r subgroup, A, B or C at infinity, a
 * public signal not below r.  proofs: n x 256 bytes, A 64 | B 128 | C 64 (the layout of zk_proof); publics: n x nPublic x
 * 32 bytes little-endian standard form (may be NULL when nPublic = 0).  The return value tells only whether the call ran.
 * Proofs go through the device in chunks of ZKHIP_VERIFY_CHUNK (2^16 otherwise): the device memory held does not grow
 * with n.  Calls on one key are serialised.  Each proof gets its own verdict from its own equation; nothing is batched by random
 * combination here (zk_vkey_verify_batch below does that, and still gives each proof its own verdict). */
#define ZK_VERIFY_OK 0
#define ZK_VERIFY_INVALID 1
#define ZK_VERIFY_MALFORMED 2
int zk_vkey_verify(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, uint8_t *verdict);

/* Two routes to the same verdicts and bytes.  Up to ZKHIP_VERIFY_COOP_MAX proofs (zk_vkey_verify) or ZKHIP_PAIRING_COOP_MAX
 * groups (zk_pairing) a call runs one workgroup per proof or group, which is what a lone proof needs; larger calls run a
 * lane per proof, which is what a batch needs.  Both variables are decimal, read at every call; 0: never cooperative;
 * anything that is not a number from 0 to 2^24 is an error of the call. */
#define ZK_VERIFY_PATH_LANES 0   /* a lane per proof: k_verify_check / _miller / _final */
#define ZK_VERIFY_PATH_COOP  1   /* a workgroup per proof: k_verify_coop */
typedef struct {
    uint32_t coop_max;        /* the threshold the last call used */
    uint32_t last_path;       /* ZK_VERIFY_PATH_* of the last zk_vkey_verify on this key */
    uint32_t last_launches;   /* kernel launches of that call */
    uint32_t reserved;
    uint64_t proofs_coop, proofs_lanes;   /* totals since zk_vkey_create */
} zk_vkey_plan;
int zk_vkey_info(zk_vkey *vk, zk_vkey_plan *plan);
int zk_pairing_last_path(void);   /* ZK_VERIFY_PATH_* of this thread's last zk_pairing, -1 before the first */

/* Batch verification by random linear combination, every proof's own verdict kept.  Arguments, layouts, verdict codes and
 * the return convention are zk_vkey_verify's.  Inside a chunk of ZKHIP_VERIFY_CHUNK proofs, consecutive proofs form groups
 * of ZKHIP_VERIFY_GROUP (decimal, 1 to 2^24, read at every call, anything else is an error of the call; 1024 otherwise; a
 * group never straddles a chunk and a chunk's last group may be short).  Malformed proofs are found first, by zk_vkey_verify's
 * criteria, get MALFORMED and take no part in any sum.  With a scalar r_i per proof, R = sum r_i, S_j = sum r_i pub_ij,
 * X = R IC_0 + sum S_j IC_j and Cs = sum r_i C_i over a group's well-formed proofs, the group passes iff
 *     prod_i e(r_i A_i, B_i) e(-R alpha, beta) e(-X, gamma) e(-Cs, delta) = 1:
 * one Miller loop and two 128-bit G1 multiplications per proof, one final exponentiation per group.  A passing group gives
 * OK to its well-formed proofs.  The well-formed proofs of a failing group are verified one by one by zk_vkey_verify's own
 * code (all failed groups of a chunk in one pass), which gives each OK or INVALID.  So a valid proof always gets OK, and an
 * INVALID one gets OK only if its group passes, which at most one of the 2^128 - 1 values of its scalar allows: with
 * scalars the prover cannot foresee, a probability of at most 1 / (2^128 - 1) per group.
 * scalars16 is FOR TESTS ONLY: n x 16 bytes little-endian, r_i of proof i; a zero scalar is an error of the call.  NULL:
 * the library draws them with getrandom() after the call has its inputs, 16 bytes each, redrawn while zero.  Scalars an
 * adversary knows or can predict before fixing the proofs are unsound: two wrong proofs whose errors cancel under those
 * scalars (r_i d_i + r_j d_j = 0) pass as a group and both get OK.  Never pass constants, counters or a seeded generator.
 * report (may be NULL; set report->size = sizeof first, as for zk_zkey_verify_report): groups counts the groups with at
 * least one well-formed proof, the ones whose equation was evaluated; proofs_rechecked the proofs sent through the
 * per-proof code; launches every kernel launch of the call.  In zk_vkey_plan a batch call leaves last_path =
 * ZK_VERIFY_PATH_BATCH and last_launches = report->launches; rechecked proofs ran on the per-proof paths and count in
 * proofs_lanes / proofs_coop, the others in neither.  The lines of beta are made by a key's first batch call. */
#define ZK_VERIFY_PATH_BATCH 2   /* the last call on the key was zk_vkey_verify_batch */
typedef struct {
    uint32_t size;              /* sizeof, set by the caller */
    uint32_t group;             /* the group size the call used */
    uint64_t groups, groups_failed;
    uint64_t proofs_rechecked;  /* well-formed proofs of failed groups, sent through the per-proof path */
    uint64_t malformed;
    uint32_t launches, reserved;
} zk_vkey_batch_report;
int zk_vkey_verify_batch(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, const uint8_t *scalars16, uint8_t *verdict,
                         zk_vkey_batch_report *report /* may be NULL */);

/* A key set: proofs under many keys in one call.  A set is a handle over existing zk_vkey objects of one device (n_keys >= 1;
 * keys on two devices are an error that names both; a key may appear twice).  The keys are borrowed, not copied: the set
 * keeps a device array with one record per key (the addresses of its IC, of its line tables and of its Miller value of
 * (alpha, beta), and its nPublic), so a key must outlive every set that names it.  zk_vkey_set_verify gives proof i the
 * verdict zk_vkey_verify gives it under key key_of[i] (the same checks, equation and codes; a proof under the wrong key of
 * the same nPublic is INVALID, not an error), and the number of kernel launches of a call depends neither on n_keys nor
 * on how the proofs are spread over the keys.  proofs: n x 256 bytes as for zk_vkey_verify; key_of: n indices below n_keys;
 * publics: the signals of proof 0, then of proof 1, ...: proof i contributes nPublic(key_of[i]) x 32 bytes, a key without
 * public signals nothing; publics_bytes must be that total (publics may be NULL when it is 0).  Errors of the call, found
 * before any launch: a key_of entry out of range (the message names the first index), a wrong publics_bytes (expected and
 * given), a null argument.  The return value tells only whether the call ran; n = 0 is a successful no-op.
 * ZKHIP_VERIFY_COOP_MAX and ZKHIP_VERIFY_CHUNK are read at every call with zk_vkey_verify's meaning and error rules: up to
 * the threshold a workgroup per proof in one launch (k_set_coop), above it a lane per proof in chunks (k_set_check /
 * _miller / _final, three launches a chunk), the device memory held not growing with n.  On the lane path the host groups
 * a chunk's proofs by key and pads every key's run to whole waves (at most 63 idle lanes per key and chunk), so a wave has
 * one key; verdicts return to the caller's positions.  Calls on one set are serialised by the set's own mutex; the keys'
 * device data never changes after zk_vkey_create, so no key's mutex is taken and every key's zk_vkey_plan is left as it
 * was.  Not here: more than one device.
 * zk_vkey_set_info: set plan->size = sizeof first, as for zk_vkey_batch_report. */
typedef struct zk_vkey_set zk_vkey_set;
typedef struct {
    uint32_t size;              /* sizeof, set by the caller */
    uint32_t n_keys;
    uint32_t last_path;         /* ZK_VERIFY_PATH_COOP or _LANES of the last zk_vkey_set_verify on this set, _BATCH after zk_vkey_set_verify_batch */
    uint32_t last_launches;     /* kernel launches of that call */
    uint64_t last_waves_padded; /* waves of that call with idle lanes: key runs that did not end on a wave border; 0 on the cooperative path */
    uint64_t proofs_coop, proofs_lanes;   /* totals since zk_vkey_set_create */
} zk_vkey_set_plan;
int zk_vkey_set_create(zk_vkey_set **out, zk_vkey *const *keys, uint32_t n_keys);
void zk_vkey_set_destroy(zk_vkey_set *set);
int zk_vkey_set_verify(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t n,
                       uint8_t *verdict);
int zk_vkey_set_info(zk_vkey_set *set, zk_vkey_set_plan *plan);

/* Batch verification across a key set: zk_vkey_verify_batch's random combination over proofs under many keys, every
 * proof's own verdict kept.  Layouts, verdict codes, the errors found before any launch and the return convention are
 * zk_vkey_set_verify's.  Inside a chunk of ZKHIP_VERIFY_CHUNK proofs the proofs are ordered by key (keys rising, a key's
 * proofs in the caller's order); in that order consecutive proofs form groups.  A group closes when it holds
 * ZKHIP_VERIFY_GROUP proofs (zk_vkey_verify_batch's switch and error rules), and also when the next proof would bring a key
 * beyond the ZKHIP_VERIFY_GROUP_KEYS-th distinct key into it (decimal, 1 to 65536, read at every call, anything else is
 * an error of the call; 1 otherwise, the measured default: groups of one key each, all keys still in one launch set;
 * DESIGN.md section 25 has the sweep).  The proofs of one key inside one group are a segment; a group never straddles
 * a chunk, a key's run may straddle groups and chunks.  Malformed proofs are found first, by zk_vkey_verify's criteria, get
 * MALFORMED and take no part in any sum.  With a scalar r_i per proof, over the well-formed proofs of segment s (key k)
 * R_s = sum r_i, S_sj = sum r_i pub_ij, X_s = R_s IC_0 + sum_j S_sj IC_(j+1) and Cs_s = sum r_i C_i, and the group passes iff
 *     prod_i e(r_i A_i, B_i) prod_s [ e(-R_s alpha_k, beta_k) e(-X_s, gamma_k) e(-Cs_s, delta_k) ] = 1:
 * one Miller loop and two 128-bit G1 multiplications per proof, three table walks per segment, one final exponentiation
 * per group.  A passing group gives OK to its well-formed proofs.  The well-formed proofs of all failing groups of a chunk
 * are verified one by one by zk_vkey_set_verify's own code in one pass, which gives each OK or INVALID.  So a valid proof
 * always gets OK, and an INVALID one gets OK only if its group passes: with scalars the prover cannot foresee, a
 * probability of at most 1 / (2^128 - 1) per group, whatever keys the group's proofs belong to.
 * scalars16 is FOR TESTS ONLY, as for zk_vkey_verify_batch: n x 16 bytes little-endian, r_i of proof i; a zero scalar is
 * an error of the call that names its index.  NULL: the library draws them with getrandom() per chunk, after the call has
 * its inputs.  Scalars an adversary knows or can predict before fixing the proofs are unsound: wrong proofs whose errors
 * cancel under those scalars, under one key or across two keys of one group, pass and all get OK.  Never pass constants,
 * counters or a seeded generator.
 * report (may be NULL; set report->size = sizeof first): groups and segments count those with at least one well-formed
 * proof, the ones evaluated; launches every kernel launch of the call.  In zk_vkey_set_plan a batch call leaves last_path
 * = ZK_VERIFY_PATH_BATCH, last_launches = report->launches and last_waves_padded = 0; rechecked proofs count in
 * proofs_coop / proofs_lanes, the others in neither.  The set's first batch call makes alpha and the lines of beta of
 * every key on the device in one launch (19 KiB a key), from bytes copied when the set was made: as for
 * zk_vkey_set_verify, the set's mutex alone is taken and every key's zk_vkey_plan is left as it was. */
typedef struct {
    uint32_t size;                 /* sizeof, set by the caller */
    uint32_t group, group_keys;    /* the two limits the call used */
    uint32_t launches;
    uint64_t groups, groups_failed, segments;   /* groups / segments with a well-formed proof */
    uint64_t proofs_rechecked, malformed;
} zk_vkey_set_batch_report;
int zk_vkey_set_verify_batch(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t n,
                             const uint8_t *scalars16 /* tests only; NULL: getrandom inside the call */,
                             uint8_t *verdict, zk_vkey_set_batch_report *report /* may be NULL */);

/* ---- Powers of Tau: check (is the .ptau a sequence of powers of one tau, are its Lagrange sections its own) ---- */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is the arithmetic half of snarkjs `powersoftau verify`.  The contribution transcript (section 7) is not read.
 * Points are in the .ptau encoding (affine Montgomery, all-zero = infinity); scalars are 32 bytes LE in standard form and
 * must be below r.  Points go through the device in chunks of ZKHIP_PTAU_CHUNK points (2^22 otherwise), so n is not
 * bound by the HBM.  device -1: the current one.
 * out[i] = 1 if G2 point i is in the order-r subgroup of the twist (infinity: 1), 0 if it is on the twist but outside.  A
 * point off the twist or with a coordinate not below q is an error naming the lowest such index.  The test is
 * [x+1] Q + psi([x] Q) + psi^2([x] Q) = psi^3([2x] Q) (x = 4965661367192848881, psi the twist's Frobenius map), exact
 * for BN254; ZKHIP_SUBGROUP_PLAIN=1 computes the same bytes by [r] Q (the yardstick of the timing tool). */
int zk_g2_in_subgroup(uint8_t *out, const uint8_t *points, uint64_t n, int32_t device);
/* out = sum_(i<n) s^(first_exp + i) points[i], affine.  The scalars are made on the device, chunk by chunk.  Every point is
 * checked as zk_g1_lagrange checks it (an error naming the lowest index); infinity is legal; n = 0 gives infinity. */
int zk_g1_power_msm(uint8_t out[64], const uint8_t *points, uint64_t n, const uint8_t s[32], uint64_t first_exp, int32_t device);
int zk_g2_power_msm(uint8_t out[128], const uint8_t *points, uint64_t n, const uint8_t s[32], uint64_t first_exp, int32_t device);
/* out[j] = sum_(i < 2^log_n) s^i w^(ij), j < 2^log_n: the forward DFT of the powers of s, 32 bytes LE standard form, w
 * the 2^log_n-th root of unity of zk_fr_ntt, log_n <= 28.  Exact for every s < r (0, 1 and s w^j = 1 included). */
int zk_fr_power_dft(uint8_t *out, const uint8_t s[32], uint32_t log_n, int32_t device);
/* The whole file.  sec[k] / sec_bytes[k]: section k of the mapped file (k = 2 .. 6 and 12 .. 15; NULL = absent). */
typedef struct zk_ptau_file_view {
    uint32_t power;
    const void *sec[16];
    uint64_t sec_bytes[16];
} zk_ptau_file_view;              /* indices 2..6, 12..15 used; NULL = absent */
typedef struct zk_ptau_check_sizes_t {
    uint32_t prepared;            /* 1: sections 12 to 15 are there and will be checked */
    uint64_t chunk_points;        /* points per chunk in effect */
    uint64_t device_bytes;        /* an upper estimate of the HBM the check holds */
} zk_ptau_check_sizes_t;
typedef struct zk_ptau_report {
    uint32_t verdict;             /* 0 OK, 1 INVALID, 2 MALFORMED */
    uint32_t failed;              /* bit k set: the equation of section k (2,3,4,5,6) failed; bit 0: a generator */
    uint32_t lagrange_failed[4];  /* sections 12..15: bit p set = level p failed */
    uint32_t bad_section;
    uint32_t bad_kind;            /* 1 coordinate >= q, 2 off curve, 3 not in subgroup, 4 infinity */
    uint64_t bad_index;
} zk_ptau_report;
/* Checks the view without touching a device: power 1 .. 28 (1 .. 27 for a prepared file: level power + 1 of section 12
 * needs a 2^(power+1)-th root of unity), a missing section, "ptau section N is short: ... bytes, power P needs ...", and
 * a file with some but not all of sections 12 to 15. */
int zk_ptau_check_sizes(const zk_ptau_file_view *ptau, zk_ptau_check_sizes_t *sizes);
/* The check.  s32: the scalar of the random combination (2 <= s < r), NULL: drawn from getrandom() after the view is
 * given, which is what makes the check sound; a fixed one is for tests.  OK exactly when
 *   every coordinate is below q, every point on its curve, no point of sections 2 to 6 at infinity, every G2 point of
 *   sections 3, 6 and 13 in the subgroup (else MALFORMED, naming section, kind and the lowest index of the first such
 *   section in the order 2, 3, 4, 5, 6, 12, 13, 14, 15; no equation is evaluated then);
 *   tauG1[0] = G1 and tauG2[0] = G2 (bit 0 of `failed`);
 *   each of sections 2, 4, 5 is a sequence of powers of the tau of tauG2[1], section 3 of the tau of tauG1[1], and section
 *   6 holds the beta of betaTauG1[0] (bits 2 .. 6 of `failed`; probability of a wrong pass below 2^29 / r);
 *   every level of sections 12 to 15, when they are there, is the Lagrange form of its powers (lagrange_failed).
 * Every failing equation is reported, not the first.  Free HBM is checked before anything is allocated.  The return
 * value tells only whether the call ran. */
int zk_ptau_check(const zk_ptau_file_view *ptau, const uint8_t *s32, int32_t device, zk_ptau_report *report);

/* ---- Powers of Tau: contribute (n points times n scalars; tau^i, alpha tau^i, beta tau^i onto a .ptau) ---- */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is the arithmetic of snarkjs `powersoftau new` / `powersoftau contribute`.
 * The operator: out[i] = scalars[i] points[i].  Points in the .ptau / .zkey encoding (affine Montgomery, all-zero =
 * infinity, which stays all-zero), scalars 32 bytes LE each in standard form, as zk_g1_scale takes its one.  A scalar >= r
 * is an error naming the lowest such index ("zk_g1_mul_vec: scalar 5 is not below r"), found before a device is touched.
 * Every point is checked before it is used: coordinates below q, on its curve and, in G2, in the order-r subgroup (the
 * endomorphism the kernel uses is a multiplication by a constant only there); one that fails is an error naming the
 * lowest such index and what is wrong, "zk_g2_mul_vec: point 37 is not in the subgroup".  n = 0 is legal.  The points go
 * through the device in chunks (ZKHIP_PTAU_CONTRIB_CHUNK=<points> in the environment sets their length, 2^20
 * otherwise) on two buffer sets, so n is not bound by the HBM.  Each lane splits its scalar by BN254's endomorphism
 * (zk_glv_split) and runs 128 doublings instead of 254; ZKHIP_MULVEC_PLAIN=1 computes the same bytes by the plain 254-bit
 * double-and-add (the yardstick of the timing tool).  device -1: the current one. */
int zk_g1_mul_vec(uint8_t *out, const uint8_t *points, const uint8_t *scalars, uint64_t n, int32_t device);
int zk_g2_mul_vec(uint8_t *out, const uint8_t *points, const uint8_t *scalars, uint64_t n, int32_t device);
/* out[i] = factor base^(first_exp + i) points[i]: the same with scalars made on the device, so that none crosses PCIe.
 * base and factor: 32 bytes LE standard form, below r.  first_exp + n must not exceed 2^64. */
int zk_g1_power_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t base[32], uint64_t first_exp, const uint8_t factor[32], int32_t device);
int zk_g2_power_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t base[32], uint64_t first_exp, const uint8_t factor[32], int32_t device);
/* What a lane makes of its scalar, on the host (the same code; no device): k = k1 + k2 lambda (mod r) with
 * 0 < k1, k2 < 2^128, 16 bytes LE each (lambda = 4407920970296243842393367215006156084916469457145843978461).  k >= r is an
 * error. */
int zk_glv_split(const uint8_t k[32], uint8_t k1[16], uint8_t k2[16]);
/* The contribution to a .ptau that is not yet prepared for phase 2: the view's sections 2 to 6 (zk_ptau_file_view; one
 * that has any of sections 12 to 15 is refused: contribute before `ptauprepare`). */
typedef struct zk_ptau_contrib_sizes {
    uint64_t tau_g1_bytes, tau_g2_bytes, alpha_tau_g1_bytes, beta_tau_g1_bytes, beta_g2_bytes;   /* of the output sections 2 .. 6 */
    uint64_t chunk_points;        /* points per chunk in effect */
    uint64_t device_bytes;        /* HBM the call holds: two buffer sets of one chunk each, of the larger group */
} zk_ptau_contrib_sizes;
typedef struct zk_ptau_contrib_out {
    uint8_t *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1, *beta_g2;                             /* sections 2, 3, 4, 5, 6 */
} zk_ptau_contrib_out;
/* Checks the view without touching a device: a power outside 1 .. 28, a prepared file, a missing section, "ptau section N
 * is short: ... bytes, power P needs ...". */
int zk_ptau_contribute_sizes(const zk_ptau_file_view *ptau, zk_ptau_contrib_sizes *sizes);
/* tauG1[i] <- tau^i tauG1[i] (i < 2^(power+1) - 1), tauG2[i] <- tau^i tauG2[i], alphaTauG1[i] <- alpha tau^i alphaTauG1[i],
 * betaTauG1[i] <- beta tau^i betaTauG1[i] (i < 2^power) with zk_g*_power_scale's kernel, chunk by chunk (the caller
 * buffers may be a mapping of the output file), betaG2 <- beta betaG2 on the host (the code of zk_g2_mul).  tau, alpha,
 * beta: 32 bytes LE standard form; 0 and values >= r are errors.  Free HBM is checked before anything is allocated.  A point
 * that is malformed (as above; in a .ptau infinity is malformed too) is an error naming its section and index, "ptau
 * section 4: point 5 is not on the curve".  The three scalars, the table of squarings of tau on the device and everything
 * derived from them are zeroed in host and device memory before the call returns; no message of zk_last_error contains
 * them.  Section 7 (the contribution transcript) is the caller's: this is arithmetic, not a ceremony protocol. */
int zk_ptau_contribute(const zk_ptau_file_view *ptau, const uint8_t tau[32], const uint8_t alpha[32], const uint8_t beta[32], int32_t device,
                       zk_ptau_contrib_out *out);

/* ---- Is this .zkey the key of this circuit over this Powers of Tau file ------------------ */
/* Nothing in the reference corresponds to these entry points (it reads a finished .zkey, src/main_prover.cpp:57-72); the
 * counterpart is the arithmetic half of snarkjs `zkey verify circuit.r1cs pot.ptau circuit.zkey`.  Section 10 of the key
 * (the contribution transcript) is NOT read: a key that passes is the circuit's key over this .ptau for SOME delta; that
 * anybody honest contributed to that delta is not shown.  No second key is made: with one scalar s, p_w = s^w over the
 * wires, and a = A'.p, b = B.p, c = C.p (row sums over the domain; A' = A plus the public-input rows), the sum
 * sum_w s^w (key point of wire w) of every section equals a multi-scalar multiplication of a Lagrange level of the .ptau by
 * a, b or c.  Every item is a polynomial identity in s of degree < 2^29: a wrong key passes one with probability < 2^29 / r.
 * zk_zkey_verify_view: the prover's view of the key plus what it does not read, gamma2 and section 3 (IC). */
typedef struct zk_zkey_verify_view {
    zk_zkey_view key;
    const void *vk_gamma2;                  /* G2, section 2 */
    const void *pointsIC;                   /* section 3: (nPublic + 1) x G1 */
    uint64_t pointsIC_bytes;
} zk_zkey_verify_view;
/* the named items: bits of `failed` and `not_checked` */
enum {
    ZK_ZV_ALPHA1 = 0, ZK_ZV_BETA1, ZK_ZV_BETA2,   /* section 2 equals alphaTauG1[0], betaTauG1[0], betaG2 of the .ptau (bytes) */
    ZK_ZV_GAMMA2,                                 /* gamma2 is the G2 generator, what snarkjs writes */
    ZK_ZV_DELTA,                                  /* e(delta1, G2) e(-G1, delta2) = 1 */
    ZK_ZV_COEFS,                                  /* section 4 against the circuit (zk_r1cs_match_zkey) */
    ZK_ZV_A, ZK_ZV_B1, ZK_ZV_B2,                  /* sum s^w A_w = MSM(T12, a); B1: (T12, b); B2: (T13, b) in G2 */
    ZK_ZV_IC,                                     /* sum_(w <= nPublic) s^w IC_w = MSM(T15, a_pub) + MSM(T14, b_pub) + MSM(T12, c_pub) */
    ZK_ZV_C,                                      /* e(sum_(w > nPublic) s^w C_w, delta2) e(-K_priv, G2) = 1 */
    ZK_ZV_H,                                      /* e(sum s^i H_i, delta2) e(-sum s^i T12'[2i + 1], G2) = 1 */
    ZK_ZV_ITEMS
};
/* the shapes of the three files that must agree: bits of `shape_failed` */
enum { ZK_ZV_SHAPE_NVARS = 0, ZK_ZV_SHAPE_NPUBLIC, ZK_ZV_SHAPE_DOMAIN, ZK_ZV_SHAPE_PTAU_UNPREPARED, ZK_ZV_SHAPE_PTAU_POWER };
typedef struct zk_zkey_verify_sizes_t {
    uint32_t log_domain;          /* k: the key's domain is 2^k; when that cannot hold the circuit (shape_failed), the smallest
                                   * k >= 1 with 2^k >= nConstraints + nPublic + 1 */
    uint32_t shape_failed;        /* what zk_zkey_verify would report without touching a device; 0: the files fit */
    uint64_t chunk_points;        /* points per chunk in effect (ZKHIP_ZKEY_VERIFY_CHUNK, 2^22 otherwise) */
    uint64_t device_bytes;        /* an upper estimate of the HBM the check holds */
} zk_zkey_verify_sizes_t;
/* Set rep->size = sizeof(zk_zkey_verify_report) before the call (only `size` bytes are written). */
typedef struct zk_zkey_verify_report {
    uint32_t size;
    uint32_t verdict;             /* 0 OK, 1 INVALID, 2 MALFORMED */
    uint32_t failed;              /* bit ZK_ZV_*: the item does not hold */
    uint32_t not_checked;         /* bit ZK_ZV_C, ZK_ZV_H: not evaluated because delta failed */
    uint32_t shape_failed;        /* bit ZK_ZV_SHAPE_*: the files do not fit each other (verdict 1, nothing else evaluated) */
    uint32_t bad_section;         /* MALFORMED: the lowest-numbered section of the key (2, 3, 5 .. 9) with a bad point, */
    uint32_t bad_kind;            /*   its kind (1 coordinate >= q, 2 off curve, 3 not in subgroup, 4 infinity) */
    uint64_t bad_index;           /*   and its lowest index (section 2: alpha1, beta1, beta2, gamma2, delta1, delta2 = 0 .. 5) */
    uint64_t coef_rows_differing; /* rows of A and B in which section 4 and the circuit differ */
    uint32_t coef_first_row;      /* the lowest such row; UINT32_MAX: none */
    uint32_t delta_is_generator;  /* delta2 is the G2 generator: a phase-2 starting key, not safe to prove with */
} zk_zkey_verify_report;
/* Checks the three views against each other without touching a device.  Errors: a null section, a section shorter than
 * the key's header implies, a .r1cs section that does not walk, a Lagrange section shorter than the .ptau's power needs, a
 * domain above 2^27.  Shapes that disagree between well-formed files (nVars, nPublic, a domain that is no power of two or
 * below nConstraints + nPublic + 1, a .ptau that is not prepared or of a power below k) are no error: they are reported in
 * shape_failed.  device_bytes: the term arrays of the
 * circuit (zk_r1cs_create and zk_r1cs_match_zkey), the masked powers, six Fr vectors over the domain, levels k of
 * sections 12 to 15 and level k + 1 of section 12, and two chunked multiplication engines (G1 and G2). */
int zk_zkey_verify_sizes(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, const zk_zkey_verify_view *zkey, zk_zkey_verify_sizes_t *sizes);
/* The check.  s32: the scalar (2 <= s < r), NULL: drawn from getrandom() after the views are given, which is what makes
 * the check sound; a fixed one is for tests.  First every point of the key's sections 2, 3 and 5 to 9 is checked as
 * zk_ptau_check checks a file's: coordinates below q, on the curve or twist, the G2 points of section 7 and beta2, gamma2,
 * delta2 in the subgroup (ZKHIP_SUBGROUP_PLAIN honoured); infinity is legal in sections 3 and 5 to 9 and not in section 2.
 * A bad point gives MALFORMED and no equation is evaluated.  Then every item of ZK_ZV_* is evaluated and every one that
 * fails is reported; when delta fails, C and H are reported in not_checked.  The .ptau's own levels are taken on trust
 * (zk_ptau_check answers for them).  Key sections go through the device in chunks on the engines of zk_ptau_check; chunk
 * sums are added on the host.  Free HBM is checked against zk_zkey_verify_sizes' estimate before anything is allocated.
 * The return value tells only whether the call ran. */
int zk_zkey_verify(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, const zk_zkey_verify_view *zkey, const uint8_t *s32, int32_t device,
                   zk_zkey_verify_report *report);

/* ---- KZG polynomial commitments over a .ptau ---------------------------------------------- */
/* Nothing in the reference corresponds to these entry points (it proves Groth16 only); the counterpart is the commitment
 * layer of snarkjs's PLONK and fflonk provers, which read the same .ptau: section 2 holds [tau^i] G1, section 3 holds
 * [tau^i] G2 and section 12 holds [L_j(tau)] G1.
 * Encodings.  Points are in the .ptau / .zkey encoding: affine Montgomery, x | y, 64 bytes in G1, all-zero = infinity.
 * Scalars (coefficients, evaluations, points z, values y) are 32 bytes little-endian in STANDARD form and must be below r.
 * Bases.  ZK_KZG_MONOMIAL: coeffs[i] is the coefficient of X^i and the bases are section 2's points.  ZK_KZG_LAGRANGE:
 * coeffs[j] is the value at w^j, w the 2^lagrange_log_n-th root of unity of zk_fr_ntt, and the bases are level
 * lagrange_log_n of section 12, the convention of zk_g1_lagrange: a Lagrange commitment of evaluations equals the monomial
 * commitment of their zk_fr_ntt(.., inverse).
 *
 * The operator: q[0 .. n - 2] = the coefficients of (p(X) - p(z)) / (X - z) and y = p(z) for p = sum coeffs[i] X^i, in one
 * pass on the device (q_(n-2) = c_(n-1), q_(i-1) = c_i + z q_i, y = c_0 + z q_0).  n = 0 is an error, "zk_fr_poly_divide: n
 * is 0"; n = 1 writes y only (q may be NULL).  "zk_fr_poly_divide: coefficient 5 is not below r" and "zk_fr_poly_divide: z is
 * not below r" are found before a device is touched.  ZKHIP_KZG_SEG=<coefficients a lane folds> (decimal, 1 to 4096, read at
 * every call, 16 otherwise; anything else is an error of the call, "ZKHIP_KZG_SEG: a number of coefficients per lane from 1
 * to 4096 expected") changes the shape of the scan and not one byte of the result.  device -1: the current one. */
int zk_fr_poly_divide(uint8_t *q, uint8_t y[32], const uint8_t *coeffs, uint64_t n, const uint8_t z[32], int32_t device);

/* The reference string on a device.  The view points into the caller's image of the file (a mapping will do); nothing of
 * it is used after zk_kzg_create returns. */
typedef struct zk_kzg zk_kzg;
typedef struct zk_kzg_view {
    uint32_t power;                         /* of the file's header */
    const void *tau_g1;                     /* section 2 */
    uint64_t tau_g1_bytes;
    const void *tau_g2;                     /* section 3 */
    uint64_t tau_g2_bytes;
    const void *lagrange_g1;                /* section 12; NULL: the file is not prepared */
    uint64_t lagrange_g1_bytes;
} zk_kzg_view;
#define ZK_KZG_MONOMIAL 0
#define ZK_KZG_LAGRANGE 1
#define ZK_KZG_NO_LAGRANGE 0xffffffffu      /* lagrange_log_n of an object without a Lagrange level */
/* Keeps the first max_coeffs points of section 2 and, unless lagrange_log_n is ZK_KZG_NO_LAGRANGE, level lagrange_log_n
 * of section 12 (2^lagrange_log_n points), both converted once to the form the multiplication kernels read; [tau] G2
 * (point 1 of section 3) as the line table of its Miller loop, beside the G2 generator's; and the work buffers of one
 * multiplication of max_coeffs points (a call with another n re-makes them for that n and keeps those).
 * 1 <= max_coeffs <= 2^(power+1) - 1 and max_coeffs < 2^31; lagrange_log_n <= power (level power + 1 of a prepared file has
 * its top power zeroed and is not offered).  Free HBM is checked before anything is allocated.  Errors, each naming the
 * section and the lowest index:
 *   "zk_kzg_create: max_coeffs 300 is outside 1 .. 127 (power 6)", "zk_kzg_create: Lagrange level 7 is above the file's power 6",
 *   "zk_kzg_create: a Lagrange level needs a prepared file (ptau section 12 is absent)",
 *   "zk_kzg_create: ptau section 2 is short: 640 bytes, 1088 needed" (sections 3 and 12 alike),
 *   "zk_kzg_create: ptau section 2: point 0 is not the generator of G1", "... section 3: point 0 is not the generator of G2",
 *   "zk_kzg_create: ptau section 2: point 5 has a coordinate that is not below q", "... is not on the curve", "... is the point
 *   at infinity" (sections 2 and 3; infinity is legal in section 12), "zk_kzg_create: ptau section 3: point 1 is not in the
 *   subgroup" (the endomorphism test of zk_g2_in_subgroup; ZKHIP_SUBGROUP_PLAIN honoured).
 * NOT checked: that the points are the powers of ONE tau, and that the Lagrange level belongs to them.  zk_ptau_check
 * (`ptaucheck`) answers for that; an object made from a file that fails it commits to nothing.  device -1: the current one.
 * Calls on one object are serialised. */
int zk_kzg_create(zk_kzg **out, const zk_kzg_view *view, uint64_t max_coeffs, uint32_t lagrange_log_n, int32_t device);
void zk_kzg_destroy(zk_kzg *kzg);
/* Set plan->size = sizeof(zk_kzg_plan) before the call (only `size` bytes are written). */
typedef struct zk_kzg_plan {
    uint32_t size;
    uint32_t lagrange_log_n;      /* ZK_KZG_NO_LAGRANGE: none */
    uint64_t max_coeffs;
    uint64_t device_bytes;        /* HBM the object holds now */
    uint32_t seg;                 /* ZKHIP_KZG_SEG in effect */
    uint32_t last_launches;       /* kernel launches of the last commit, open, verify or verify_batch on the object */
} zk_kzg_plan;
int zk_kzg_info(zk_kzg *kzg, zk_kzg_plan *plan);
/* out[k] = sum_i coeffs[k][i] B_i for m vectors of n scalars (m x n x 32 bytes), one after another: the sort, bucket and
 * reduction kernels of zk_msm_g1 over the resident bases; only the scalars cross PCIe.  out: m x 64 bytes; an all-zero
 * vector gives the all-zero encoding.  Monomial: 1 <= n <= max_coeffs ("zk_kzg_commit: n = 200 exceeds max_coeffs = 127");
 * Lagrange: n = 2^lagrange_log_n exactly ("zk_kzg_commit: n = 32, the Lagrange level holds 64 points", "zk_kzg_commit: the
 * object holds no Lagrange level").  "zk_kzg_commit: polynomial 2, coefficient 5 is not below r" is found before a device
 * is touched; "zk_kzg_commit: n is 0", "zk_kzg_commit: basis 7 is unknown".  m = 0 is legal. */
int zk_kzg_commit(zk_kzg *kzg, uint8_t *out, const uint8_t *coeffs, uint64_t n, uint64_t m, uint32_t basis);
/* Opens m polynomials of n monomial coefficients, polynomial k at its own zs[k] (m x 32 bytes; a caller that opens several
 * polynomials at one point repeats it): ys[k] = p_k(z_k) (32 bytes) and proofs[k] = the commitment of (p_k - y_k) / (X - z_k)
 * (64 bytes; n = 1: infinity).  The quotient is made by zk_fr_poly_divide's kernels and goes into the multiplication's sort
 * without leaving the device.  Commit and open are linear: an opening proof that folds several polynomials is the
 * caller's linear combination of these.  Errors as zk_kzg_commit's, and "zk_kzg_open: z 3 is not below r". */
int zk_kzg_open(zk_kzg *kzg, uint8_t *ys, uint8_t *proofs, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs);
/* verdict[i] (ZK_VERIFY_*) of opening i: e(C_i - [y_i] G + [z_i] pi_i, G2) = e(pi_i, [tau] G2).  MALFORMED: C_i or pi_i with
 * a coordinate not below q or off the curve (infinity is legal: C = pi = infinity with y = 0 is the zero polynomial's
 * opening), z_i or y_i not below r.  INVALID: well-formed and the equation does not hold.  commitments, proofs: m x 64
 * bytes; zs, ys: m x 32 bytes.  Openings go through the device in chunks of ZKHIP_VERIFY_CHUNK (2^16 otherwise).  The
 * return value tells only whether the call ran. */
int zk_kzg_verify(zk_kzg *kzg, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m,
                  uint8_t *verdict);
/* ONE verdict byte for the batch, by random linear combination: with a 128-bit r_i != 0 per opening,
 *     e(sum r_i C_i - [sum r_i y_i] G + sum (r_i z_i) pi_i, G2) = e(sum r_i pi_i, [tau] G2)
 * (three multi-scalar multiplications, one fixed-base multiplication, one pair of Miller loops).  *verdict: MALFORMED if
 * any opening is (zk_kzg_verify's criteria; nothing is summed then), else OK if the equation holds, else INVALID.  It does
 * not say which opening failed: zk_kzg_verify does.  An all-valid batch always passes; a batch with an invalid opening
 * passes for at most one of the 2^128 - 1 values of that opening's scalar: probability <= 1 / (2^128 - 1) with scalars the
 * prover cannot foresee.  m = 0 gives OK.
 * scalars16 is FOR TESTS ONLY: m x 16 bytes little-endian; "zk_kzg_verify_batch: scalar 3 is zero" is an error of the
 * call.  NULL: the library draws them with getrandom() after the call has its inputs, redrawn while zero.  Scalars an
 * adversary knows before fixing the openings are unsound: two wrong openings whose errors cancel under them pass. */
int zk_kzg_verify_batch(zk_kzg *kzg, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m,
                        const uint8_t *scalars16, uint8_t *verdict);

/* ---- Grand products and batch inversion over Fr -------------------------------------------- */
/* Running products of scalars on the device: round 2 of a PLONK prover (the accumulator Z of the permutation argument) and
 * the batched inversion its later rounds and every lookup argument need.  Nothing in the reference corresponds to them.
 * Encodings are the KZG section's: scalars are 32 bytes little-endian in STANDARD form and must be below r, which is
 * checked before a device is touched; an error names the array and the lowest index.  Pointers are the host's; the vectors
 * are staged through the device.  device -1: the current one.  n < 2^31.
 * The formula.  With T = prod den[j], 1 / (den[0] .. den[i-1]) = (den[i] .. den[n-1]) / T, so every entry is a prefix scan,
 * a suffix scan and ONE inversion for the whole vector, and no element is inverted on its own:
 *     z[i] = (num[0] .. num[i-1]) (den[i] .. den[n-1]) / T,      1 / a[i] = (a[0] .. a[i-1]) (a[i+1] .. a[n-1]) / T.
 * ZKHIP_SCAN_SEG=<elements a lane folds> (decimal, 1 to 4096, read at every call, 8 otherwise; anything else is an error of
 * the call, "ZKHIP_SCAN_SEG: a number of elements per lane from 1 to 4096 expected") changes the shape of the scan and not
 * one byte of any result. */

/* out[i] = in[i]^-1; a zero gives zero; *zeros (may be NULL) = how many.  out == in is legal.  n = 0 is legal.
 * "zk_fr_batch_inverse: value 5 is not below r", "zk_fr_batch_inverse: n is not below 2^31". */
int zk_fr_batch_inverse(uint8_t *out, const uint8_t *in, uint64_t n, uint64_t *zeros, int32_t device);

#define ZK_SCAN_EXCLUSIVE 1u
/* inclusive: out[i] = in[0] ... in[i];  exclusive: out[0] = 1, out[i] = in[0] ... in[i-1].  Zeros are ordinary values:
 * everything from the first zero on (after it, when exclusive) is zero.  out == in is legal.  n = 0 is legal.
 * "zk_fr_prefix_product: value 5 is not below r", "zk_fr_prefix_product: flags 2 is unknown". */
int zk_fr_prefix_product(uint8_t *out, const uint8_t *in, uint64_t n, uint32_t flags, int32_t device);

/* z[0] = 1, z[i] = prod_(j<i) num[j]/den[j] (n values); last = prod_(j<n) num[j]/den[j].  A zero denominator is an
 * error of the call naming the lowest index ("zk_fr_grand_product: denominator 5 is zero"); a zero numerator is legal.
 * "zk_fr_grand_product: numerator 5 is not below r", "zk_fr_grand_product: denominator 5 is not below r".  n = 0 writes
 * last = 1 only.  The zero is found from T = 0 by a pass of its own: a call without one pays nothing for the check. */
int zk_fr_grand_product(uint8_t *z, uint8_t last[32], const uint8_t *num, const uint8_t *den, uint64_t n, int32_t device);

/* The permutation argument's accumulator over cols wire columns of n = 2^log_n rows:
 *   num_i = prod_j (wires[j][i] + beta * shifts[j] * w^i + gamma),  den_i = prod_j (wires[j][i] + beta * sigmas[j][i] + gamma),
 * w the 2^log_n-th root of zk_fr_ntt; z and last as in zk_fr_grand_product.  wires, sigmas: cols x n x 32 bytes, column
 * after column; sigmas[j][i] is the VALUE sigma_j(w^i) = shifts[j'] * w^i' of the cell that (j, i) maps to; shifts: cols x 32.
 * 1 <= cols <= 8, log_n <= 28.  last == 1 iff the copy constraints hold, up to the soundness of (beta, gamma); the call does
 * not judge it.  This is snarkjs's round-2 convention: cols = 3, shifts (1, k1, k2), Z[0] = 1.  The factors are built inside
 * the scan: no num or den vector exists on the device.  Errors: "zk_plonk_permutation_product: cols 9 is outside 1 .. 8",
 * "zk_plonk_permutation_product: log_n 29 is above 28", "zk_plonk_permutation_product: wires: column 1, row 5 is not below r"
 * (sigmas alike), "zk_plonk_permutation_product: shift 2 is not below r", "zk_plonk_permutation_product: beta is not below r"
 * (gamma alike), "zk_plonk_permutation_product: row 5 has a zero denominator" (the lowest such row).
 * NOT checked: that shifts name distinct cosets, that sigmas is a permutation. */
int zk_plonk_permutation_product(uint8_t *z, uint8_t last[32], const uint8_t *wires, const uint8_t *sigmas, uint32_t cols,
                                 uint32_t log_n, const uint8_t *shifts, const uint8_t beta[32], const uint8_t gamma[32], int32_t device);

/* ---- PLONK quotient and coset transforms --------------------------------------------------- */
/* Round 3 of a PLONK prover: the quotient t = num / Z_H from evaluations on a coset, and the coset transform it is made of.
 * Nothing in the reference corresponds to them.  Encodings are the two sections' above: scalars are 32 bytes little-endian
 * in STANDARD form and must be below r, which is checked before a device is touched; an error names the array and the
 * lowest index.  Pointers are the host's; the vectors are staged through the device.  device -1: the current one.
 * ZKHIP_QUOT_SEG=<points a lane takes> (decimal, 1 to 4096, read at every call, 16 otherwise; anything else is an error of the
 * call, "ZKHIP_QUOT_SEG: a number of points per lane from 1 to 4096 expected") changes the shape of the three kernels of
 * this section and not one byte of any result. */

/* The transform on the coset g H', H' the m = 2^log_m-th roots of unity, w_m the root zk_fr_ntt uses for m.
 * Forward (inverse == 0): in holds n_in <= m coefficients of p, out[i] = p(g w_m^i) for i < m, natural order.
 * Inverse: in holds n_in = m evaluations, out[i] = coefficient i: the inverse transform's i-th value times g^(-i).
 * shift NULL: g = 1; a forward call with n_in = m then equals zk_fr_ntt.  out == in is legal.  log_m <= 28.
 * "zk_fr_coset_ntt: log_m 29 is above 28", "zk_fr_coset_ntt: n_in 9 is outside 1 .. 2^log_m = 8", "zk_fr_coset_ntt: n_in 4 is
 * not 2^log_m = 8" (inverse), "zk_fr_coset_ntt: value 5 is not below r", "zk_fr_coset_ntt: shift is not below r",
 * "zk_fr_coset_ntt: shift is zero". */
int zk_fr_coset_ntt(uint8_t *out, const uint8_t *in, uint64_t n_in, uint32_t log_m, const uint8_t shift[32], int inverse, int32_t device);

/* What does not change from proof to proof, kept on the device: the eight circuit polynomials of a three-column PLONK
 * circuit over n = 2^log_n rows, extended once to the coset x_i = g w_4n^i, i < 4n (w_4n^4 = w, the root of round 2), the
 * extension of L1 = (X^n - 1) / (n (X - 1)), the tables of the transforms of size 4n and the work vectors of one call. */
typedef struct zk_plonk_circuit zk_plonk_circuit;
typedef struct zk_plonk_circuit_view {
    uint32_t log_n, basis;                  /* ZK_KZG_MONOMIAL: coefficients; ZK_KZG_LAGRANGE: values at w^j (what round 2 takes) */
    const uint8_t *ql, *qr, *qm, *qo, *qc, *s1, *s2, *s3;   /* n rows each */
    uint8_t k1[32], k2[32];                 /* NOT checked to give disjoint cosets, as the shifts of round 2 */
    const uint8_t *shift;                   /* NULL: 5.  Refused unless g^(4n) != 1 */
} zk_plonk_circuit_view;
/* 1 <= log_n <= 25: every transform of size 4n <= 2^27 is zk_fr_ntt's pipeline.  Free HBM is checked before anything is
 * allocated: while it is made the object holds the nine extensions twice (72 n rows), afterwards 76 n rows and the tables.
 * "zk_plonk_circuit_create: log_n 26 is outside 1 .. 25", "zk_plonk_circuit_create: basis 7 is unknown",
 * "zk_plonk_circuit_create: qm 5 is not below r" (ql, qr, qm, qo, qc, s1, s2, s3), "zk_plonk_circuit_create: k1 is not below
 * r" (k2, shift alike), "zk_plonk_circuit_create: shift is zero", "zk_plonk_circuit_create: shift^(4n) is 1: Z_H vanishes on
 * the coset".  Calls on one object are serialised. */
int zk_plonk_circuit_create(zk_plonk_circuit **out, const zk_plonk_circuit_view *v, int32_t device);
void zk_plonk_circuit_destroy(zk_plonk_circuit *c);
/* Set plan->size = sizeof(zk_plonk_circuit_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_circuit_plan {
    uint32_t size;
    uint32_t log_n;
    uint64_t points;              /* of the extension: 4n */
    uint64_t device_bytes;        /* HBM the object holds */
    uint32_t seg;                 /* ZKHIP_QUOT_SEG in effect */
    uint32_t last_launches;       /* kernel launches of zk_plonk_circuit_create or of the last zk_plonk_quotient on the object */
} zk_plonk_circuit_plan;
int zk_plonk_circuit_info(zk_plonk_circuit *c, zk_plonk_circuit_plan *plan);

/* t = num / Z_H, Z_H = X^n - 1, with
 *   num = ql a + qr b + qm a b + qo c + qc + PI
 *       + alpha [ (a + beta X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma) z(X)
 *               - (a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma) z(w X) ]
 *       + alpha^2 (z - 1) L1(X):
 * snarkjs's round-3 terms.  a, b, cc, z: the proof's polynomials by coefficients, a_len .. z_len of them (blinding by
 * multiples of Z_H makes them longer than n); pi: the n coefficients of the public-input polynomial, NULL: zero.
 * t receives 4n rows, the coefficients of t with zeros from *t_len on; *t_len is one more than the index of the highest
 * non-zero coefficient (0 for t = 0).  The quotient is made pointwise on the coset and brought back by one inverse
 * transform, which is exact iff t has at most 4n coefficients: every length is 1 .. 2n and a_len + b_len + c_len + z_len <=
 * 5n + 3 (the usual blinding, n + 2, n + 2, n + 2, n + 3, needs n >= 8).  "zk_plonk_quotient: b_len 17 is outside 1 .. 2n =
 * 16", "zk_plonk_quotient: a_len + b_len + c_len + z_len = 25 exceeds 5n + 3 = 23: t would have more than 4n coefficients",
 * "zk_plonk_quotient: z 5 is not below r" (a, b, c, z, pi), "zk_plonk_quotient: alpha is not below r" (beta, gamma alike).
 * When num is NOT divisible by Z_H (a witness that breaks a gate or a copy constraint) the call does not refuse: it returns
 * the interpolant of num / Z_H on the coset, of degree below 4n, and the caller compares *t_len with its own bound (3n - 3
 * unblinded, 3n + 6 with the usual blinding).  A t_len above the bound is a necessary sign of a bad witness, NOT a proof of
 * a good one: a remainder of very low degree can alias below the bound.  It does not replace a gate check.
 * Splitting t into t_lo, t_mid, t_hi and blinding the parts is the caller's: three slices and two coefficients. */
int zk_plonk_quotient(zk_plonk_circuit *c, uint8_t *t, uint64_t *t_len, const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len,
                      const uint8_t *cc, uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t *pi, const uint8_t alpha[32],
                      const uint8_t beta[32], const uint8_t gamma[32]);

/* ---- PLONK evaluations and opening proofs -------------------------------------------------- */
/* Rounds 4 and 5 of a PLONK prover: the six evaluations at zeta and zeta w, the linearisation polynomial and the two
 * opening proofs.  Nothing in the reference corresponds to them.  Encodings are the KZG section's: scalars are 32 bytes
 * little-endian in STANDARD form and must be below r, which is checked before a device is touched; an error names the
 * array and the lowest index; points are in the .ptau encoding, all-zero = infinity.  Pointers are the host's.  Conventions
 * are round 3's: n = 2^log_n, w zk_fr_ntt's root for n, shifts (1, k1, k2), terms weighted 1, alpha, alpha^2, Z_H = X^n - 1,
 * L1 = (X^n - 1) / (n (X - 1)).
 * ZKHIP_OPEN_SEG=<coefficients a lane takes> (decimal, 1 to 4096, read at every call, 16 otherwise; anything else is an
 * error of the call, "ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected") changes the shape of the
 * kernels of this section and not one byte of any result.  The divisions are zk_fr_poly_divide's (ZKHIP_KZG_SEG). */

/* ys[j] = p_j(zs[j]) for m polynomials of n coefficients (m x n x 32 bytes, one after another; zs, ys: m x 32 bytes): the
 * convention of zk_kzg_open without the commitment, in two launches for all m (for every 65535 of them).  n = 0 is an
 * error, "zk_fr_poly_eval: n is 0"; m = 0 is legal.  "zk_fr_poly_eval: n is not below 2^31",
 * "zk_fr_poly_eval: polynomial 2, coefficient 5 is not below r", "zk_fr_poly_eval: z 3 is not below r".
 * device -1: the current one. */
int zk_fr_poly_eval(uint8_t *ys, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs, int32_t device);

/* What rounds 4 and 5 keep on the kzg's device: the eight circuit polynomials by coefficients (ZK_KZG_LAGRANGE: converted
 * once by zk_fr_ntt's inverse transform; the view's `shift` is ignored), and room for a, b, c, z, the three parts of t, F
 * and a quotient, max_coeffs rows each.  The object BORROWS the zk_kzg, as a key set borrows its keys: its points and the
 * work buffers of its multiplication are used by zk_plonk_open; destroying the kzg before the object is the caller's error.
 * Refused before anything is allocated:
 *   "zk_plonk_opening_create: log_n 26 is outside 1 .. 25", "zk_plonk_opening_create: basis 7 is unknown",
 *   "zk_plonk_opening_create: n + 6 = 70 exceeds the kzg's max_coeffs = 64" (F of a blinded proof has n + 6 coefficients),
 *   "zk_plonk_opening_create: device 1 is not the kzg's device 0" (-1: the kzg's),
 *   "zk_plonk_opening_create: qm 5 is not below r" (ql, qr, qm, qo, qc, s1, s2, s3),
 *   "zk_plonk_opening_create: k1 is not below r" (k2 alike).
 * Free HBM is checked before anything is allocated.  Calls on one object are serialised. */
typedef struct zk_plonk_opening zk_plonk_opening;
int zk_plonk_opening_create(zk_plonk_opening **out, zk_kzg *kzg, const zk_plonk_circuit_view *v, int32_t device);
void zk_plonk_opening_destroy(zk_plonk_opening *o);
/* Set plan->size = sizeof(zk_plonk_opening_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_opening_plan {
    uint32_t size;
    uint32_t log_n;
    uint64_t device_bytes;        /* HBM the object holds (the kzg's is the kzg's) */
    uint32_t seg;                 /* ZKHIP_OPEN_SEG in effect */
    uint32_t last_launches;       /* kernel launches of the last zk_plonk_evaluate or zk_plonk_open on the object */
    uint32_t pending;             /* 1: an evaluation is pending, zk_plonk_open may follow */
    uint32_t reserved;
} zk_plonk_opening_plan;
int zk_plonk_opening_info(zk_plonk_opening *o, zk_plonk_opening_plan *plan);

/* Round 4.  evals = a(zeta) | b(zeta) | c(zeta) | s1(zeta) | s2(zeta) | z(zeta w), 32 bytes each, in that order: two
 * launches.  a, b, cc, z: the proof's polynomials by coefficients, a_len .. z_len of them, each 1 .. max_coeffs
 * ("zk_plonk_evaluate: b_len 0 is outside 1 .. max_coeffs = 70"); "zk_plonk_evaluate: z 5 is not below r" (a, b, c, z),
 * "zk_plonk_evaluate: zeta is not below r".  The four vectors, zeta and the six values stay in the object for round 5: an
 * evaluation is then PENDING (a later zk_plonk_evaluate replaces it). */
int zk_plonk_evaluate(zk_plonk_opening *o, uint8_t evals[6 * 32], const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, const uint8_t *cc,
                      uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t zeta[32]);

/* Round 5.  With a' = a(zeta), b', c', s1', s2', z'w = z(zeta w) of the pending evaluation and t = t_lo + X^n t_mid + X^2n t_hi:
 *   r(X) = a' b' qM + a' qL + b' qR + c' qO + PI(zeta) + qC
 *        + alpha [ (a' + beta zeta + gamma)(b' + beta k1 zeta + gamma)(c' + beta k2 zeta + gamma) z(X)
 *                - (a' + beta s1' + gamma)(b' + beta s2' + gamma)(c' + beta s3(X) + gamma) z'w ]
 *        + alpha^2 (z(X) - 1) L1(zeta)
 *        - Z_H(zeta) (t_lo + zeta^n t_mid + zeta^2n t_hi)
 *   F(X)    = r + v a + v^2 b + v^3 c + v^4 s1 + v^5 s2
 *   w_zeta       = commit( (F - F(zeta)) / (X - zeta) )
 *   w_zeta_omega = commit( (z - z'w) / (X - zeta w) )
 *   E       = v a' + v^2 b' + v^3 c' + v^4 s1' + v^5 s2'
 *   r_zeta  = r(zeta) = F(zeta) - E
 * F is one pass over 15 rows, the divisions are zk_fr_poly_divide's kernels (F(zeta) is the first one's remainder) and the
 * multiplications zk_kzg_commit's over the kzg's resident points, under the kzg's mutex: F and both quotients never leave
 * the device.  pi_zeta NULL: 0.  f NULL: F is not wanted; otherwise f receives max_coeffs rows, F's coefficients with zeros
 * from *f_len on, *f_len the largest of the lengths of the rows F is made of (n + 6 with the usual blinding).  zeta^n = 1 is
 * legal: Z_H(zeta) = 0, and L1(zeta) is 1 for zeta = 1, else 0.  The parts of t: 1 .. max_coeffs coefficients each,
 * "zk_plonk_open: mid_len 0 is outside 1 .. max_coeffs = 70"; "zk_plonk_open: t_lo 5 is not below r" (t_lo, t_mid, t_hi),
 * "zk_plonk_open: alpha is not below r" (beta, gamma, v, pi_zeta alike).  Without a pending evaluation the call is refused,
 * "zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first"; a call whose arguments pass consumes it.
 * r_zeta = 0 exactly when the round-3 identity holds at zeta; the call returns it and does not judge it.
 * NOT checked: that r(zeta) = 0; that the t parts are the split of the round-3 quotient; that k1 and k2 give disjoint cosets.
 * Blinding the parts of t is the caller's. */
int zk_plonk_open(zk_plonk_opening *o, uint8_t w_zeta[64], uint8_t w_zeta_omega[64], uint8_t r_zeta[32], uint8_t *f, uint64_t *f_len, const uint8_t *t_lo,
                  uint64_t lo_len, const uint8_t *t_mid, uint64_t mid_len, const uint8_t *t_hi, uint64_t hi_len, const uint8_t pi_zeta[32],
                  const uint8_t alpha[32], const uint8_t beta[32], const uint8_t gamma[32], const uint8_t v[32]);

/* ---- PLONK prover and verifier ------------------------------------------------------------- */
/* The five rounds above chained on the device, the Fiat-Shamir transcript that draws their challenges, and the verifier
 * of the proofs they make.  Nothing in the reference corresponds to them; the counterpart is snarkjs's PLONK prover and
 * verifier for a three-column circuit.  Encodings are the sections' above: scalars are 32 bytes little-endian in STANDARD
 * form and must be below r; points are in the .ptau encoding (affine, Montgomery, 64 bytes, all-zero = infinity).
 * Conventions are rounds 2 to 5's: n = 2^log_n, w zk_fr_ntt's root for n, shifts (1, k1, k2), Z[0] = 1, terms weighted
 * 1, alpha, alpha^2, Z_H = X^n - 1, L1 = (X^n - 1) / (n (X - 1)).  The knobs of the rounds (ZKHIP_SCAN_SEG, ZKHIP_QUOT_SEG,
 * ZKHIP_OPEN_SEG, ZKHIP_KZG_SEG) shape the kernels of a proof and change not one byte of it; the prover's own kernels (the
 * wire gather, the blinding, the split of t) follow ZKHIP_QUOT_SEG.
 *
 * The transcript.  The hash is Keccak-256 with the ORIGINAL padding byte 0x01 (Ethereum's), not SHA-3's 0x06.  What is
 * hashed: a scalar as 32 bytes BIG-endian, standard form; a point as x | y, 32 bytes big-endian standard form each,
 * infinity as 64 zero bytes.  A challenge is the digest read as a big-endian integer, reduced mod r.
 *   beta  = H([qM], [qL], [qR], [qO], [qC], [s1], [s2], [s3], publics[0 .. n_public), [a], [b], [c])
 *   gamma = H(beta)
 *   alpha = H(beta, gamma, [z])
 *   zeta  = H(alpha, [t_lo], [t_mid], [t_hi])
 *   v     = H(zeta, a', b', c', s1', s2', z'w)
 *   u     = H([W_zeta], [W_zeta_omega])
 * The order follows snarkjs 0.7's; no file made by snarkjs was at hand, so parity with snarkjs is UNPINNED. */

/* out32 = Keccak-256(data[0 .. len)).  No device.  Keccak-256("") = c5d24601 86f7233c 927e7db2 dcc703c0 e500b653 ca82273b
 * 7bfad804 5d85a470; Keccak-256("abc") = 4e03657a ea45a94f c7d47ba8 26c8d667 c0d1e6e3 3a64a036 ec44f58f a12d6c45. */
int zk_keccak256(uint8_t out32[32], const uint8_t *data, uint64_t len);

#define ZK_PLONK_PROOF_BYTES 768   /* [a] [b] [c] [z] [t_lo] [t_mid] [t_hi] [W_zeta] [W_zeta_omega], 64 bytes each, then
                                    * a' b' c' s1' s2' z'w, 32 bytes each */
#define ZK_PLONK_BLINDS 11

/* What a verifier needs.  The commitments in the transcript's order. */
typedef struct zk_plonk_vkey {
    uint32_t size;                /* set to sizeof(zk_plonk_vkey) before zk_plonk_prover_vkey */
    uint32_t log_n;
    uint64_t n_public;
    uint8_t k1[32], k2[32];
    uint8_t qm[64], ql[64], qr[64], qo[64], qc[64], s1[64], s2[64], s3[64];
    uint8_t tau_g2[128];          /* [tau] G2, the .ptau encoding */
} zk_plonk_vkey;

/* A prover for one circuit on the kzg's device.  view: the eight vectors as zk_plonk_circuit_create and
 * zk_plonk_opening_create take them.  a_map, b_map, c_map: n indices each, row i's wires are witness[a_map[i]],
 * witness[b_map[i]], witness[c_map[i]].  The object BORROWS the kzg as a zk_plonk_opening does, and keeps on its device: the
 * maps, s1 .. s3 by values (round 2), what a zk_plonk_circuit keeps for round 3 (the extensions), what a zk_plonk_opening
 * keeps for rounds 4 and 5 (the coefficients), and room for a witness and a proof's vectors.  It makes the eight commitments once.
 * 3 <= log_n <= 25 (the usual blinding needs 3n + 6 <= 4n), n + 6 <= the kzg's max_coeffs, n_public <= n, n_witness >= 1.
 * Refused before a device is touched:
 *   "zk_plonk_prover_create: log_n 2 is outside 3 .. 25", "zk_plonk_prover_create: basis 7 is unknown",
 *   "zk_plonk_prover_create: n + 6 = 70 exceeds the kzg's max_coeffs = 64",
 *   "zk_plonk_prover_create: n_public 9 exceeds n = 8", "zk_plonk_prover_create: n_witness is 0",
 *   "zk_plonk_prover_create: device 1 is not the kzg's device 0" (-1: the kzg's),
 *   "zk_plonk_prover_create: b_map 5 is 12, not below n_witness = 12" (a_map, b_map, c_map; the lowest row),
 *   "zk_plonk_prover_create: qm 5 is not below r" (ql, qr, qm, qo, qc, s1, s2, s3), "zk_plonk_prover_create: k1 is not below r"
 *   (k2, shift alike), "zk_plonk_prover_create: shift is zero", "zk_plonk_prover_create: shift^(4n) is 1: Z_H vanishes on the
 *   coset".  Free HBM is checked before anything is allocated.  Calls on one object are serialised. */
typedef struct zk_plonk_prover zk_plonk_prover;
int zk_plonk_prover_create(zk_plonk_prover **out, zk_kzg *kzg, const zk_plonk_circuit_view *view, const uint32_t *a_map, const uint32_t *b_map,
                           const uint32_t *c_map, uint64_t n_witness, uint64_t n_public, int32_t device);
void zk_plonk_prover_destroy(zk_plonk_prover *p);
int zk_plonk_prover_vkey(zk_plonk_prover *p, zk_plonk_vkey *vk);
/* Set plan->size = sizeof(zk_plonk_prover_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_prover_plan {
    uint32_t size;
    uint32_t log_n;
    uint64_t n_witness, n_public;
    uint64_t device_bytes;        /* HBM the object holds (the kzg's is the kzg's) */
    uint32_t scan_seg, quot_seg, open_seg, kzg_seg;   /* the knobs in effect */
    uint32_t last_launches;       /* kernel launches of the last zk_plonk_prove on the object (of the creation before it) */
    uint32_t round_launches[5];   /* of them, round 1 .. round 5 (the multiplications of a round's commitments with it).  Both
                                   * counts are differences of the library's one process-wide launch counter, as every *_info's
                                   * last_launches: launches other threads make meanwhile, on any object, are counted in */
} zk_plonk_prover_plan;
int zk_plonk_prover_info(zk_plonk_prover *p, zk_plonk_prover_plan *plan);

/* proof (ZK_PLONK_PROOF_BYTES) from a witness of n_witness scalars.  publics: n_public scalars; PI takes the value
 * -publics[i] at w^i and 0 elsewhere (NULL with n_public = 0).  blind: NULL, or ZK_PLONK_BLINDS scalars b1 .. b11 (FOR TESTS:
 * a proof with known blinds hides nothing); with NULL they are drawn from the OS generator (getrandom).  Any value below r is
 * legal, 0 included.  The usual blinding:
 *   a += (b1 X + b2) Z_H,  b += (b3 X + b4) Z_H,  c += (b5 X + b6) Z_H,  z += (b7 X^2 + b8 X + b9) Z_H,
 *   t_lo + b10 X^n,  t_mid - b10 + b11 X^n,  t_hi - b11.
 * The witness is uploaded once; after that only commitments, the six values, `last`, t's length, r(zeta) and the challenges
 * cross PCIe.  "zk_plonk_prove: witness 5 is not below r" (publics, blind alike), refused before a device is touched.
 * A bad witness is refused and NO proof byte is written: "zk_plonk_prove: the copy constraints do not hold" (round 2's
 * last != 1), "zk_plonk_prove: the witness does not satisfy the gates" (t has more than 3n + 6 coefficients, or r(zeta) != 0),
 * "zk_plonk_prove: a denominator of the permutation product is zero" (probability about 3n / r over beta, gamma). */
int zk_plonk_prove(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *witness, const uint8_t *publics, const uint8_t *blind);

/* MANY WITNESSES A CALL.  m witnesses of the prover's circuit give m proofs, proof i byte for byte what zk_plonk_prove gives
 * witness i with blinds i.  The proofs of a CHUNK of B advance through the five rounds in lock-step and every round's
 * commitments for the whole chunk are ONE multiplication: four multiplications a chunk whatever it holds, against nine a proof.
 * B is ZKHIP_PLONK_PROVE_BATCH, 1 .. ZK_PLONK_MANY_MAX_BATCH ("ZKHIP_PLONK_PROVE_BATCH: a number of proofs from 1 to 64
 * expected" is an error of the call before any work); unset, the default for the circuit's size, which DESIGN.md section 36
 * states with its measurement.  m proofs take ceil(m / B) chunks.  With B = 1 the call is a loop of zk_plonk_prove's own five
 * rounds and keeps nothing more on the device.
 * Layout: proofs m x ZK_PLONK_PROOF_BYTES; status m words; witnesses m x n_witness scalars back to back; publics m x n_public
 * scalars back to back (NULL with n_public = 0); blinds NULL (drawn from the OS generator and wiped from the host and the
 * device when the call leaves) or m x ZK_PLONK_BLINDS scalars, FOR TESTS as zk_plonk_prove's.  m = 0 is accepted and touches
 * no device.
 * A proof that cannot be made does not take the others with it: status[i] is ZK_PLONK_MANY_MADE or why proof i was refused,
 * the 768 bytes of a refused proof are left untouched, its vectors are zeros in every later multiplication of its chunk, and
 * the call still returns 0.  zk_last_error() then holds the refusal of the LOWEST refused index with that index:
 *   "zk_plonk_prove_many: proof 3: the copy constraints do not hold", "zk_plonk_prove_many: proof 3: witness 5 is not below r"
 *   (publics, blind alike).
 * The entry returns non-zero only for errors of the call: "null argument", a bad knob, out of memory, "zk_plonk_prove_many: m is
 * not below 2^31", and a chunk width the multiplication cannot take, checked before anything is allocated and naming the
 * width that would fit:
 *   "zk_plonk_prove_many: a chunk of 64 proofs is too large: 3 x 64 x 1048582 scalars x 13 windows = 2617260672 >= 2^31 table
 *   rows; ZKHIP_PLONK_PROVE_BATCH=52 would fit" (>= 2^32 sort entries alike),
 *   "zk_plonk_prove_many: out of memory (a chunk of 16 proofs needs 301234 MiB of HBM, 250000 MiB free);
 *   ZKHIP_PLONK_PROVE_BATCH=12 would fit".
 * On the device the first call with B > 1 makes, and the object keeps: a table with a row per window over the kzg's first
 * n + 6 points (the kzg's mutex is held only while its points are copied), B slots (a proof's witness, publics, blinds, wire
 * values, z, PI, t and its nine committed rows of n + 6) and the multiplication's buffers for 3 B vectors.  A call with another
 * B makes them again.  The call holds the object's mutex throughout and does not use the kzg's multiplication. */
#define ZK_PLONK_MANY_MAX_BATCH 64
#define ZK_PLONK_MANY_MADE 0
#define ZK_PLONK_MANY_ZERO_DENOMINATOR 1   /* a denominator of the permutation product is zero */
#define ZK_PLONK_MANY_COPIES 2             /* the copy constraints do not hold */
#define ZK_PLONK_MANY_GATES 3              /* the witness does not satisfy the gates (t's length, or r(zeta) != 0) */
#define ZK_PLONK_MANY_NOT_BELOW_R 4        /* a value of the witness, the publics or the blinds is not below r */
int zk_plonk_prove_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *witnesses, const uint8_t *publics,
                        const uint8_t *blinds);
/* The same from m circom witnesses of nVars = nWires values each, back to back: each is checked as zk_plonk_prove_r1cs checks
 * its one and extended on its slot; its publics are its values 1 .. n_public.  "witness has 5 values, the r1cs 7 wires" and
 * "zk_plonk_prove_r1cs_many: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)" are errors of the call. */
int zk_plonk_prove_r1cs_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *wtns, uint32_t nVars, const uint8_t *blinds);
/* The multiplication's own entry: k >= 1 polynomials of n + 6 coefficients each, back to back (shorter ones padded with
 * zeros), give k commitments, out k x 64 bytes in the .ptau encoding, each what zk_kzg_commit gives.  3 B vectors a
 * multiplication, B as above (the table and the buffers are made for B = 1 too).  A polynomial of zeros gives infinity.
 * "zk_plonk_prover_commit_many: vector 2 coefficient 5 is not below r", "zk_plonk_prover_commit_many: k is 0". */
int zk_plonk_prover_commit_many(zk_plonk_prover *p, uint8_t *out, const uint8_t *coeffs, uint64_t k);
/* Set plan->size = sizeof(zk_plonk_prover_many_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_prover_many_plan {
    uint32_t size;
    uint32_t batch;               /* B in effect for the next call */
    uint32_t table_batch;         /* the B the table, the slots and the buffers were made for; 0: not made */
    uint32_t window_bits;         /* of the table: what make_msm_plan chooses for a batch of 3 B vectors of n + 6 */
    uint32_t table_rows;          /* rows of n + 6 points, one a window */
    uint32_t reserved;
    uint64_t table_bytes, slot_bytes, msm_bytes;   /* HBM of the table, the slots, the multiplication's buffers */
    uint32_t last_chunks;         /* of the last zk_plonk_prove_many, _r1cs_many or _commit_many on the object */
    uint32_t last_multiplications;   /* 4 a chunk with B > 1; 9 a proof made with B = 1 */
    uint32_t last_launches;       /* kernel launches, a difference of the process-wide counter as every last_launches */
    uint32_t last_drains;         /* times the host waited for the stream: 4 a chunk and, a proof, the looped cores' (the scan, t's
                                   * length, the six values, F(zeta)) */
    uint32_t last_refused;        /* proofs of the call whose status is not 0 */
    uint32_t reserved2;
} zk_plonk_prover_many_plan;
int zk_plonk_prover_many_info(zk_plonk_prover *p, zk_plonk_prover_many_plan *plan);

/* *verdict = ZK_VERIFY_OK / ZK_VERIFY_INVALID / ZK_VERIFY_MALFORMED for one proof under vk with n_public = vk->n_public
 * publics.  MALFORMED: a point of the proof that is not on the curve (or a coordinate not below q), or one of the six values
 * or a public input not below r.  Otherwise the transcript is recomputed, u included, and with
 *   r0 = alpha (a' + beta s1' + gamma)(b' + beta s2' + gamma)(c' + gamma) z'w + alpha^2 L1(zeta) - PI(zeta)
 *   D  = a' b' [qM] + a' [qL] + b' [qR] + c' [qO] + [qC]
 *      + (alpha (a' + beta zeta + gamma)(b' + beta k1 zeta + gamma)(c' + beta k2 zeta + gamma) + alpha^2 L1(zeta) + u) [z]
 *      - alpha (a' + beta s1' + gamma)(b' + beta s2' + gamma) beta z'w [s3] - Z_H(zeta) ([t_lo] + zeta^n [t_mid] + zeta^2n [t_hi])
 *   F  = D + v [a] + v^2 [b] + v^3 [c] + v^4 [s1] + v^5 [s2]
 *   E  = (r0 + v a' + v^2 b' + v^3 c' + v^4 s1' + v^5 s2' + u z'w) [1]
 * the verdict is OK iff e(W_zeta + u W_zeta_omega, [tau]G2) = e(zeta W_zeta + u zeta w W_zeta_omega + F - E, G2).  The
 * multiplications are the host's (zk_g1_mul, 18 of them), the pairing product one lane of zk_kzg_verify's kernel over the
 * kzg's line tables: "zk_plonk_verify: the key's [tau]G2 is not the kzg's".  A bad KEY is an error of the call, not a verdict:
 * "zk_plonk_verify: vk->size is not sizeof(zk_plonk_vkey)", "zk_plonk_verify: log_n 2 is outside 3 .. 25",
 * "zk_plonk_verify: n_public 9 exceeds n = 8", "zk_plonk_verify: k1 is not below r" (k2 alike),
 * "zk_plonk_verify: a commitment of the key is not a point of the curve". */
int zk_plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *publics, uint8_t *verdict);

/* A verifier made from the KEY ALONE, for many proofs a call: no zk_kzg and no .ptau, since a verifier needs the eight
 * commitments and [tau]G2 and the key holds both.  On its device the object keeps the line tables of the G2 generator and of
 * [tau]G2, the eight commitments and the generator of G1, the Keccak state after the key's commitments (the 512 bytes every
 * round-1 message begins with: three blocks permuted, 13 words of the fourth absorbed), and, from the first call on, the
 * buffers of one chunk of proofs.  A bad key is refused as zk_plonk_verify refuses it, before a device is touched:
 *   "zk_plonk_verifier_create: vk->size is not sizeof(zk_plonk_vkey)", "zk_plonk_verifier_create: log_n 2 is outside 3 .. 25",
 *   "zk_plonk_verifier_create: n_public 9 exceeds n = 8", "zk_plonk_verifier_create: k1 is not below r" (k2 alike),
 *   "zk_plonk_verifier_create: a commitment of the key is not a point of the curve";
 * and, on the device, as zk_ptau_check judges section 3 (coordinates below q, the twist, the subgroup; infinity is refused):
 *   "zk_plonk_verifier_create: the key's [tau]G2 is not a point of the twist in the subgroup".
 * Free HBM is checked before anything is allocated.  Calls on one object are serialised.
 *
 * THE KEY FILE (host/vkjson.hpp, PlonkVKey.to_json / from_json, the programs plonkvkey and plonkverifier) has the field names of
 * snarkjs's verification_key.json for PLONK: protocol "plonk", curve "bn128", nPublic, power, k1, k2, Qm Ql Qr Qo Qc S1 S2 S3,
 * X_2, w; points as decimal strings, projective with z = 1 (infinity: 0 1 0).  It names a key of THIS project's compile and
 * transcript: parity with snarkjs is UNPINNED, so a key made by snarkjs parses (when its w is this library's root for its
 * power), but proofs made by snarkjs are not promised to verify. */
typedef struct zk_plonk_verifier zk_plonk_verifier;
int zk_plonk_verifier_create(zk_plonk_verifier **out, const zk_plonk_vkey *vk, int32_t device);
void zk_plonk_verifier_destroy(zk_plonk_verifier *v);
/* Set plan->size = sizeof(zk_plonk_verifier_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_verifier_plan {
    uint32_t size;
    uint32_t log_n;
    uint64_t n_public;
    uint64_t device_bytes;        /* HBM the object holds, the buffers of a chunk included once a call has made them */
    uint64_t chunk;               /* ZKHIP_PLONK_VERIFY_CHUNK in effect */
    uint32_t last_launches;       /* kernel launches of the last call on the object (of the creation before it) */
    uint32_t last_chunks;         /* chunks of the last call with m > 0: ceil(m / min(m, chunk)) */
} zk_plonk_verifier_plan;
int zk_plonk_verifier_info(zk_plonk_verifier *v, zk_plonk_verifier_plan *plan);
/* verdict[i] = what zk_plonk_verify gives proof i (proofs: m x ZK_PLONK_PROOF_BYTES) with publics[i] (m x n_public x 32 bytes,
 * proof-major; NULL when n_public = 0): ZK_VERIFY_OK / ZK_VERIFY_INVALID / ZK_VERIFY_MALFORMED, with the same malformed
 * conditions; the point at infinity is a point, so a proof that holds one is judged by the equation.  Everything per proof
 * runs on the device, four launches a chunk: the checks, the transcript and the scalars (a lane per proof); the nineteen
 * products (a lane per product); L and W (a lane per proof); zk_kzg_verify's pairing kernel over the object's tables.  A
 * malformed proof does not disturb its neighbours.  m = 0 is legal and does nothing; "zk_plonk_verifier_verify: m is not below
 * 2^31".  ZKHIP_PLONK_VERIFY_CHUNK=<proofs a chunk> (decimal, 1 to 2^20, read at every call, 65536 otherwise; anything else is
 * an error of the call, "ZKHIP_PLONK_VERIFY_CHUNK: a number of proofs from 1 to 2^20 expected") bounds the HBM of a call, about
 * 4.2 KB + 32 n_public bytes a proof, and changes no verdict. */
int zk_plonk_verifier_verify(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *verdict);
/* The first kernel alone, for tests of the device transcript on inputs that are no valid proofs and for whoever looks for
 * the first difference against another implementation's transcript: challenges[i] = beta gamma alpha zeta v u of proof i, 6 x
 * 32 bytes little-endian in standard form; status[i] = 0, or ZK_VERIFY_MALFORMED with the row left all zero.  "m is not
 * below 2^31" and the knob as above, under this entry's name. */
int zk_plonk_verifier_challenges(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *challenges, uint8_t *status);

/* Batch verification by random linear combination, every proof's own verdict kept.  Arguments, layouts, verdict codes, m = 0,
 * "zk_plonk_verifier_verify_batch: m is not below 2^31" and ZKHIP_PLONK_VERIFY_CHUNK are zk_plonk_verifier_verify's.  Inside a
 * chunk, consecutive proofs form groups of ZKHIP_PLONK_VERIFY_GROUP (decimal, 1 to 2^20, read at every call, 65536 otherwise;
 * anything else is an error of the call, "ZKHIP_PLONK_VERIFY_GROUP: a number of proofs from 1 to 2^20 expected"; a group never
 * straddles a chunk and a chunk's last group may be short).  Malformed proofs are found first, by the transcript kernel's own
 * checks, get MALFORMED and take no part in any sum; a group of malformed proofs alone evaluates no equation.  Every
 * well-formed proof i asks e(L_i, G2) = e(W_i, [tau]G2) with L_i = sum_(t < 18) s_it B_it and W_i = W_zeta,i + u_i
 * W_zeta_omega,i: nine bases F_t that all proofs share (the key's eight commitments and the generator) and the proof's own
 * nine points P_ij.  With a scalar r_i per proof, over a group's well-formed proofs
 *     S_t = sum_i r_i s_it (t < 9, in Fr),   L = sum_t S_t F_t + sum_i sum_j (r_i s_i,9+j) P_ij,
 *     W = sum_i r_i W_zeta,i + (r_i u_i) W_zeta_omega,i,
 * and the group passes iff e(L, G2) e(-W, [tau]G2) = 1: no pairing per proof, eleven points per proof in two bucket
 * multiplications per group, the scalars made and folded on the device, one cooperative pairing product per group.  A
 * passing group gives OK to its well-formed proofs.  The well-formed proofs of a failing group are verified one by one by
 * zk_plonk_verifier_verify's own kernels from the status and scalars already on the device (all failed groups of a chunk
 * before the chunk's verdicts leave), which gives each OK or INVALID.  So a valid proof always gets OK, and an INVALID one
 * gets OK only if its group passes, which at most one of the 2^128 - 1 values of its scalar allows: with scalars the prover
 * cannot foresee, a probability of at most 1 / (2^128 - 1) per group.  A batch with many invalid proofs pays the
 * combination and then the per-proof code for every failing group: use zk_plonk_verifier_verify, or a smaller group
 * (profiles/plonk_verify_batch_timing.txt, 65536 proofs: 21 ms all valid against zk_plonk_verifier_verify's 89 ms; with ONE
 * invalid proof 107 ms in one group of 65536 and 78 ms in groups of 16384; with 1 % invalid every group fails at every size).
 * scalars16 is FOR TESTS ONLY: m x 16 bytes little-endian, r_i of proof i; a zero scalar is an error of the call,
 * "zk_plonk_verifier_verify_batch: scalar 3 is zero".  NULL: the library draws them with getrandom() after the call has its
 * inputs, 16 bytes each, redrawn while zero.  Scalars an adversary knows or can predict before fixing the proofs are unsound:
 * two wrong proofs whose errors cancel under those scalars (r_i d_i + r_j d_j = 0) pass as a group and both get OK.  Never
 * pass constants, counters or a seeded generator.
 * report (may be NULL; set report->size = sizeof first, as for zk_vkey_batch_report): group is the group size the call used,
 * min(the knob, the chunk's capacity); groups counts the groups with at least one well-formed proof, the ones whose equation
 * was evaluated; proofs_rechecked the well-formed proofs sent through the per-proof kernels; launches every kernel launch of
 * the call.  After a batch call zk_plonk_verifier_info reports last_launches = report->launches and the call's chunks.  The
 * batch buffers (about 1.4 KB a proof, the two multiplications' workspaces, and the nine fixed bases in the bucket kernels'
 * form) are made by the object's first batch call, after the free HBM has been checked, and count in device_bytes. */
typedef struct {
    uint32_t size;              /* sizeof, set by the caller */
    uint32_t group;             /* the group size the call used */
    uint64_t groups, groups_failed;
    uint64_t proofs_rechecked, malformed;
    uint32_t launches, chunks;
} zk_plonk_batch_report;
int zk_plonk_verifier_verify_batch(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *verdict,
                                   zk_plonk_batch_report *report /* may be NULL */);
/* FOR TESTS: sums[g] = L | W of group g (128 bytes, the file's form; 128 zero bytes for a group with no well-formed proof),
 * in the order the groups are formed; n_groups = the number written.  No pairing is run.  scalars16 must be given;
 * "zk_plonk_verifier_batch_sums: sums_cap 2 is below the call's 3 groups". */
int zk_plonk_verifier_batch_sums(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *sums,
                                 uint64_t sums_cap, uint64_t *n_groups);

/* A verifier over a KEY SET: proofs under many keys in one call, proof i under key key_of[i].  PLONK's setup is universal, so
 * the keys of a service share one [tau]G2, and a group of proofs under any number of keys is still ONE equation
 * e(L, G2) e(-W, [tau]G2) = 1.  The set keeps on its device one pair of line tables and the generator of G1 once, and per key a
 * record of what the transcript needs and the eight commitments; from the first call on, the buffers of one chunk.
 * zk_plonk_verifier_set_create COPIES the keys and borrows nothing.  n_keys is 1 to 65536 ("zk_plonk_verifier_set_create: n_keys
 * 0 is outside 1 .. 65536"; "zk_plonk_verifier_set_create: key 2 is null"); a key may appear twice; keys may differ in log_n,
 * n_public, k1, k2 and their commitments.  Every key is checked as zk_plonk_verifier_create checks it, with the same texts
 * under this entry's name and the key's index, before a device is touched:
 *   "zk_plonk_verifier_set_create: key 3: vk->size is not sizeof(zk_plonk_vkey)", "zk_plonk_verifier_set_create: key 3: log_n 2 is
 *   outside 3 .. 25", "zk_plonk_verifier_set_create: key 3: n_public 9 exceeds n = 8", "zk_plonk_verifier_set_create: key 3: k1 is
 *   not below r" (k2 alike), "zk_plonk_verifier_set_create: key 3: a commitment of the key is not a point of the curve";
 * all keys must carry the same tau_g2 bytes, "zk_plonk_verifier_set_create: key 3's [tau]G2 is not key 0's"; and [tau]G2 is
 * classified on the device once: "zk_plonk_verifier_set_create: the keys' [tau]G2 is not a point of the twist in the subgroup".
 * Free HBM is checked before anything is allocated.  Calls on one set are serialised. */
typedef struct zk_plonk_verifier_set zk_plonk_verifier_set;
int zk_plonk_verifier_set_create(zk_plonk_verifier_set **out, const zk_plonk_vkey *const *vks, uint32_t n_keys, int32_t device);
void zk_plonk_verifier_set_destroy(zk_plonk_verifier_set *set);
/* Set plan->size = sizeof(zk_plonk_verifier_set_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_verifier_set_plan {
    uint32_t size;
    uint32_t n_keys;
    uint64_t max_n_public;        /* the largest n_public of the set's keys */
    uint64_t device_bytes;        /* HBM the set holds, the buffers of a chunk and of a batch call included once made */
    uint64_t chunk;               /* ZKHIP_PLONK_VERIFY_CHUNK in effect */
    uint32_t last_launches;       /* kernel launches of the last call on the set */
    uint32_t last_chunks;         /* chunks of the last call with m > 0 */
} zk_plonk_verifier_set_plan;
int zk_plonk_verifier_set_info(zk_plonk_verifier_set *set, zk_plonk_verifier_set_plan *plan);
/* verdict[i] = what zk_plonk_verifier_verify gives proof i under key key_of[i]: the same checks, equation and codes, so a proof
 * under the wrong key of the same n_public is INVALID, not an error.  publics is RAGGED, as for zk_vkey_set_verify: proof i
 * contributes n_public(key_of[i]) x 32 bytes, back to back in the proofs' order; publics_bytes must be their total and publics
 * may be NULL when that is 0.  Found before any launch: "zk_plonk_verifier_set_verify: key_of[5] = 9, the set holds 4 keys" (the
 * first such index), "zk_plonk_verifier_set_verify: publics_bytes: 640 expected (20 values of 32 bytes), 608 given",
 * "zk_plonk_verifier_set_verify: m is not below 2^31", a null argument.  m = 0 is legal and does nothing.
 * ZKHIP_PLONK_VERIFY_CHUNK keeps its meaning and its error.  Inside a chunk the proofs are ORDERED BY KEY, keys rising and a
 * key's proofs in the caller's order, through an index array the kernels read (proofs and publics are uploaded as the caller
 * holds them): the lanes of a wave then mostly share a key, and with it the transcript's loop over the publics and the base of
 * a fixed term.  Verdicts return to the caller's positions.  Four launches a chunk, whatever n_keys is and however the proofs
 * spread over the keys. */
int zk_plonk_verifier_set_verify(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                                 uint8_t *verdict);
/* zk_plonk_verifier_verify_batch over the set: in the key-ordered chunk, consecutive proofs form groups of
 * ZKHIP_PLONK_VERIFY_GROUP (the knob, default and error of that entry); there is NO limit on the keys of a group.  A SEGMENT is the
 * proofs of one key inside one group; a key's run may straddle groups and chunks, a group never straddles a chunk.  Malformed
 * proofs get MALFORMED and take no part in any sum.  With a scalar r_i per proof, over a group's well-formed proofs
 *     S_G   = sum_i r_i s_i,G                                  (the generator's term, the whole group)
 *     S_s,t = sum_(i in segment s) r_i s_it,  t < 8            (the eight commitments F_k(s),t of the segment's key)
 *     L = S_G G + sum_s sum_(t < 8) S_s,t F_k(s),t + sum_i sum_(j < 9) (r_i s_i,9+j) P_ij,
 *     W = sum_i r_i W_zeta,i + (r_i u_i) W_zeta_omega,i,
 * and the group passes iff e(L, G2) e(-W, [tau]G2) = 1: a further key in a group costs eight more points of the bucket
 * multiplication.  A passing group gives OK to its well-formed proofs; the well-formed proofs of all failing groups of a chunk
 * go through the set's per-proof kernels from the status and scalars already on the device, before the chunk's verdicts
 * leave.  So a valid proof always gets OK, and an invalid one gets OK with probability at most 1 / (2^128 - 1) a group, whatever
 * keys the group holds.  scalars16 is FOR TESTS ONLY (m x 16 bytes, r_i of proof i in the caller's order); a zero scalar is
 * an error, "zk_plonk_verifier_set_verify_batch: scalar 3 is zero"; NULL: the library draws them with getrandom() after the call
 * has its inputs.  Scalars an adversary knows or can predict before fixing the proofs are unsound: two wrong proofs whose
 * errors cancel under those scalars pass as a group and both get OK, AND THE TWO MAY STAND UNDER TWO DIFFERENT KEYS of one
 * group, since the group is one equation.  Never pass constants, counters or a seeded generator.
 * report (may be NULL; set report->size = sizeof first): groups and segments count those with at least one well-formed proof.
 * The batch buffers and the keys' commitments in the bucket kernels' form are made by the set's first batch call, after the
 * free HBM has been checked, and count in device_bytes. */
typedef struct {
    uint32_t size;              /* sizeof, set by the caller */
    uint32_t group;             /* the group size the call used: min(the knob, the chunk's capacity) */
    uint32_t launches, chunks;
    uint64_t groups, groups_failed;
    uint64_t segments;
    uint64_t proofs_rechecked, malformed;
} zk_plonk_set_batch_report;
int zk_plonk_verifier_set_verify_batch(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes,
                                       uint64_t m, const uint8_t *scalars16, uint8_t *verdict, zk_plonk_set_batch_report *report /* may be NULL */);
/* FOR TESTS: sums[g] = L | W of group g (128 bytes, the file's form; 128 zero bytes for a group with no well-formed proof), in
 * the order the groups are formed; n_groups = the number written.  No pairing is run.  scalars16 must be given;
 * "zk_plonk_verifier_set_batch_sums: sums_cap 2 is below the call's 3 groups". */
int zk_plonk_verifier_set_batch_sums(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                                     const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap, uint64_t *n_groups);

/* ---- PLONK from an R1CS ---------------------------------------------------------------------- */
/* A circom .r1cs compiled on the device to what zk_plonk_prover_create takes: the five selectors, the three wire maps and the
 * permutation s1 s2 s3; the extension of a circom witness by the wires the compile introduces; and a prover made from the
 * compiled circuit.  Nothing in the reference corresponds to them; the counterpart is snarkjs's `plonk setup`, whose layout
 * this follows in spirit only: the layout below is this project's own and parity with snarkjs is UNPINNED.
 * ZKHIP_R1CS_SEG=<elements a lane takes> (decimal, 1 to 4096, read at every call, 8 otherwise; anything else is an error of the
 * call, "ZKHIP_R1CS_SEG: a number of elements per lane from 1 to 4096 expected") changes the shape of the scans of this
 * section and not one byte of any result.
 *
 * The layout.  Input: a zk_r1cs_view as zk_r1cs_create takes it (m constraints, nWires, nPublic = nPubOut + nPubIn) and k1, k2.
 * A linear combination (LC) L of A, B, C of a constraint is normalised first: terms whose coefficient is 0 are dropped; the
 * constant k_L is the coefficient of L's term on wire 0, or 0 if there is none; the other terms stay in file order, t_L of them
 * (the same non-zero wire twice is two terms).  L is then reduced to ONE term (s_L, c_L):
 *   t_L = 0: (wire 0, 0).   t_L = 1: the term itself.
 *   t_L >= 2: t_L - 1 ADDITION GATES, each introducing a new wire.  The first has a = w_1, b = w_2, c = new, ql = c_1, qr = c_2,
 *   qo = -1; each later one a = the previous new wire, b = w_i, ql = 1, qr = c_i, qo = -1; qm = qc = 0 in all of them.  The
 *   term is (the last new wire, 1).
 * Rows.  Rows 0 .. nPublic - 1 are the public rows: a = wire 1 + i, b = c = wire 0, ql = 1, everything else 0 (the prover's PI
 * is -publics[i] there).  Then, for each constraint in file order, its addition gates (A's, then B's, then C's) and its FINAL
 * GATE: a = s_A, b = s_B, c = s_C, qm = c_A c_B, ql = c_A k_B, qr = k_A c_B, qo = -c_C, qc = k_A k_B - k_C.
 *   N = nPublic + sum over the constraints of (max(t_A - 1, 0) + max(t_B - 1, 0) + max(t_C - 1, 0) + 1),
 *   log_n = max(3, ceil(log2 N)), n = 2^log_n; rows N .. n - 1 are padding: every selector 0, all three wires wire 0.
 * New wires are numbered nWires + q, q the addition gate's rank in row order; n_witness = nWires + n_additions.
 * Sigma.  Cell (col, row) has index col n + row, col 0, 1, 2 for a, b, c.  All 3n cells take part, padding included.  The
 * cells of one wire, in ascending cell index, form one cycle: each points to the next, the last to the first.
 * s_col[row] = K_col' w^row' for the cell (col', row') it points to, K = (1, k1, k2), w zk_fr_ntt's root for n.  A wire no cell
 * names has no cycle.
 * The extension.  The value of new wire nWires + q is the running sum of c_i w[wire_i] over its LC's kept terms up to the
 * gate's own (rank r: the terms 0 .. r), so that every addition gate holds.
 *
 * Refused by name before a device is touched: "zk_plonk_r1cs_create: k1 is not below r" (k2 alike), "zk_plonk_r1cs_create: k1 or
 * k2 is zero", "zk_plonk_r1cs_create: 1, k1 and k2 do not name three different cosets of the n-th roots of unity" (k1^n = 1,
 * k2^n = 1 or (k1 / k2)^n = 1, for the n of the term counts, which is at least the circuit's), "zk_plonk_r1cs_create: N =
 * 33554433 rows exceed 2^25", "zk_plonk_r1cs_create: n_witness = 4294967296 is not below 2^32", "zk_plonk_r1cs_create: nWires is
 * 0: wire 0 is the constant", "zk_plonk_r1cs_create: nPublic 4 is not below nWires = 4", the section's own texts of
 * zk_r1cs_create ("r1cs constraints section is truncated (constraint 5)").  Refused when the object is made, on the device:
 * "r1cs constraint 5: wire id >= nWires", "r1cs constraint 5: coefficient >= r" (zk_r1cs_create's), and a second kept term on
 * wire 0 in one LC, "zk_plonk_r1cs_create: constraint 5: B names wire 0 twice": the lowest constraint, A before B before C.
 * Custom gates (sections 4 and 5 of the file) are the caller's to refuse.  Calls on one object are serialised. */
typedef struct zk_plonk_r1cs zk_plonk_r1cs;
int zk_plonk_r1cs_create(zk_plonk_r1cs **out, const zk_r1cs_view *view, const uint8_t k1[32], const uint8_t k2[32], int32_t device);
void zk_plonk_r1cs_destroy(zk_plonk_r1cs *c);
/* Set plan->size = sizeof(zk_plonk_r1cs_plan) before the call (only `size` bytes are written). */
typedef struct zk_plonk_r1cs_plan {
    uint32_t size;
    uint32_t log_n;
    uint64_t rows;                /* N */
    uint64_t n_public, n_wires, n_additions, n_witness;
    uint64_t terms;               /* of the section, dropped ones included */
    uint64_t device_bytes;        /* HBM the object holds */
    uint32_t seg;                 /* ZKHIP_R1CS_SEG in effect */
    uint32_t sort_passes;         /* 8-bit digit passes of the sort of the cells: ceil(ceil(log2 n_witness) / 8) */
    uint32_t last_launches;       /* kernel launches of zk_plonk_r1cs_create, or of the last extension on the object */
    uint32_t reserved;
} zk_plonk_r1cs_plan;
int zk_plonk_r1cs_info(zk_plonk_r1cs *c, zk_plonk_r1cs_plan *plan);
/* vectors: 8 n rows of 32 bytes, ql qr qm qo qc s1 s2 s3 in zk_plonk_circuit_view's order, as VALUES over the domain
 * (ZK_KZG_LAGRANGE), standard form; a_map, b_map, c_map: n indices each. */
int zk_plonk_r1cs_circuit(zk_plonk_r1cs *c, uint8_t *vectors, uint32_t *a_map, uint32_t *b_map, uint32_t *c_map);
/* out: n_witness scalars, the nVars = nWires of a circom witness and the new wires' values after them.
 * "witness has 5 values, the r1cs 7 wires", "zk_plonk_r1cs_extend: witness 5 is not below r". */
int zk_plonk_r1cs_extend(zk_plonk_r1cs *c, uint8_t *out, const uint8_t *wtns, uint32_t nVars);

/* The prover of the section above over a compiled circuit, on the kzg's device.  It goes through zk_plonk_r1cs_circuit and
 * zk_plonk_prover_create: the 8 n rows and the maps cross the host once a circuit, and the refusals are that entry's.  The
 * prover BORROWS the compiled object as it borrows the kzg.  shift: as zk_plonk_circuit_view's.
 * "zk_plonk_prover_create_r1cs: the compiled circuit's device 1 is not the kzg's device 0". */
int zk_plonk_prover_create_r1cs(zk_plonk_prover **out, zk_kzg *kzg, zk_plonk_r1cs *compiled, const uint8_t *shift, int32_t device);
/* zk_plonk_prove from a circom witness: the nVars = nWires values are uploaded, extended on the device, the publics are
 * wtns[1 .. 1 + n_public), and the five rounds run over the resident witness.  blind: as zk_plonk_prove.  The refusals of a bad
 * witness are zk_plonk_prove's under this entry's name ("zk_plonk_prove_r1cs: the witness does not satisfy the gates"), and
 * "witness has 5 values, the r1cs 7 wires", "zk_plonk_prove_r1cs: witness 5 is not below r",
 * "zk_plonk_prove_r1cs: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)". */
int zk_plonk_prove_r1cs(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *wtns, uint32_t nVars, const uint8_t *blind);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */
