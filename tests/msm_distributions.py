"""Adversarial scalar distributions for the MSM's integer and control structure (sort, level-1 walk, merge levels, bucket
reductions), with a plain-Python model of what the sort must emit.  No GPU use; the device tests feed these to
zk_msm_sort, zk_msm_g1 / zk_msm_g2 and the prover.  The field and curve arithmetic inside the same kernels is the
business of extreme_inputs.py.

The model restates, in Python integers and numpy, three things of csrc/msm_sort.hip:
  * make_plan          = make_msm_plan + SortBufs' size rules (window width, windows, bucket sets, refusals);
  * signed_digits      = the recoding of k mod r into digits -2^(c-1) <= d < 2^(c-1), top digit >= 0;
  * sort_model         = bucket and entry word of every non-zero digit, per table mode (the paragraph at zk_msm_sort in
                         include/zkhip.h), as (offsets, entries sorted inside each bucket).

Scalars of the digit-built families are assembled from chosen window values 0 <= v_w < 2^(c-1): there is no carry, so the
device must emit exactly these digits.  B = nbuckets = 2^(c-1); the positive digits are 1 .. B - 1 (buckets 0 .. B - 2);
bucket B - 1 is reached by the digit -2^(c-1) alone, which the carry families produce.  Every family takes the plan, so
one definition serves every c, W and table mode, returns (scalars uint8[n_total, 32], facts) and ASSERTS the facts it is
named for from the model: a family that loses its property at some shape fails on the CPU."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # BN254 group order
BIN_SHIFT, BIN_MAX, BIN_SPAN, STAGE_CAP, L1_CHUNK = 11, 256, 8192, 8192, 32           # msm_sort.hip / msm_accum.hip geometry
STAIR_M = (1, 16, 31, 32, 33, 64, 160)
# most level-1 lanes one round can hold: 3 workgroups of 256 lanes on each of 256 compute units (msm_accum.hip plans 2 or 3 G1
# workgroups per unit from the occupancy calculator).  E > 32 * this leaves the minimum chunk of 32 at any occupancy up to that.
ROUND_LANES_MAX = 3 * 256 * 256


class NotApplicable(Exception):
    """The family cannot have its property at this plan (say so instead of passing vacuously)."""


# ---------------------------------------------------------------- plan
def make_plan(n, window_bits=0, table_mode=0, batch=1):
    """n scalars per vector -> dict with the fields of zk_msm_sort_plan (but `entries`)."""
    if table_mode > 2:
        raise ValueError("table mode")
    batch = batch or 1
    n1 = n if n else 1
    lg = n1.bit_length() - 1
    c = window_bits
    if table_mode:
        if c == 0:
            c = lg - 2 if lg > 2 else 2
            if lg == 20:
                c = 19
            if lg == 21:
                c = 20
            if batch > 1:
                c += 1
            c = min(c, 20)
        c = min(c, 22)
    else:
        if c == 0:
            c = lg - 6 if lg > 6 else 2
        c = min(c, 16)
    c = max(c, 2)
    W = (256 + c - 1) // c
    W255 = (255 + c - 1) // c
    if W255 < W and (R >> ((W255 - 1) * c)) + 1 < (1 << (c - 1)):
        W = W255
    B = 1 << (c - 1)
    sets = table_mode if table_mode else W
    if batch > 1:
        if table_mode != 1:
            raise ValueError("batched MSMs need a table row per window")
        sets = batch
    total = n * (batch if batch > 1 else 1)
    t1 = total if total else 1
    rows = (W + table_mode - 1) // table_mode if table_mode else 1
    if t1 * W >= 1 << 32:
        raise ValueError("n * windows >= 2^32")
    if t1 * rows >= 1 << 31:
        raise ValueError("table rows >= 2^31")
    return dict(c=c, W=W, sets=sets, nbuckets=B, total_buckets=sets * B, table_mode=table_mode, batch=batch if batch > 1 else 1,
                n=total, max_entries=t1 * W)


def n_per_vector(plan):
    return plan["n"] // plan["batch"]


def bin_shift(plan):
    sh = BIN_SHIFT
    while ((plan["total_buckets"] + (1 << sh) - 1) >> sh) > BIN_MAX:
        sh += 1
    return sh


def top_max(plan):
    """largest value of the top window that keeps a scalar below r whatever the windows below hold"""
    return (R >> ((plan["W"] - 1) * plan["c"])) - 1


# ---------------------------------------------------------------- scalars <-> windows
def pack_windows(vals, c):
    """vals int64[n, W], 0 <= v < 2^c  ->  (uint8[n, 32] little-endian, overflow: bool[n] bits at or above 2^256)"""
    n, W = vals.shape
    limbs = np.zeros((n, (W * c + 31) // 32 + 2), dtype=np.uint64)
    v = vals.astype(np.uint64)
    for w in range(W):
        p = c * w
        x = v[:, w] << np.uint64(p % 32)                 # < 2^(22 + 31)
        limbs[:, p // 32] += x & np.uint64(0xffffffff)   # windows occupy disjoint bits: no limb overflows
        limbs[:, p // 32 + 1] += x >> np.uint64(32)
    assert (limbs >> np.uint64(32) == 0).all()
    over = (limbs[:, 8:] != 0).any(axis=1)
    return np.ascontiguousarray(limbs[:, :8].astype("<u4")).view(np.uint8).reshape(n, 32), over


def unpack_windows(sc, c, W):
    """uint8[n, 32] -> raw window values int64[n, W]"""
    n = sc.shape[0]
    limbs = np.zeros((n, 8 + 2), dtype=np.uint64)
    limbs[:, :8] = np.ascontiguousarray(sc).view("<u4").reshape(n, 8)
    out = np.zeros((n, W), dtype=np.int64)
    for w in range(W):
        p = c * w
        if p >= 256:
            break
        x = limbs[:, p // 32] | (limbs[:, p // 32 + 1] << np.uint64(32))
        out[:, w] = ((x >> np.uint64(p % 32)) & np.uint64((1 << c) - 1)).astype(np.int64)
    return out


def to_ints(sc):
    return [int.from_bytes(row.tobytes(), "little") for row in sc]


def from_ints(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(len(ks), 32).copy()


def reduce_mod_r(sc):
    """every row below r (rows whose top byte could reach r's are taken through Python integers)"""
    sc = sc.copy()
    for i in np.nonzero(sc[:, 31] >= (R >> 248))[0]:
        sc[i] = from_ints([int.from_bytes(sc[i].tobytes(), "little") % R])[0]
    return sc


def signed_digits_int(k, c, W):
    """the recoding on one Python integer (any 256-bit value): the reference the vectorised one is tested against"""
    k %= R
    out, carry = [], 0
    for w in range(W):
        d = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if d >= 1 << (c - 1) else 0
        out.append(d - (carry << c))
    assert carry == 0
    return out


def signed_digits(sc, plan):
    """uint8[n, 32] (any 256-bit values) -> int64[n, W]"""
    c, W = plan["c"], plan["W"]
    raw = unpack_windows(reduce_mod_r(sc), c, W)
    carry = np.zeros(raw.shape[0], dtype=np.int64)
    for w in range(W):
        d = raw[:, w] + carry
        carry = (d >= 1 << (c - 1)).astype(np.int64)
        raw[:, w] = d - (carry << c)
    assert not carry.any(), "top digit negative: the plan's W is too small"
    return raw


def digits_value_matches(D, sc, plan):
    """sum_w D[i, w] 2^(c w) == k_i mod r for every i (exact where the borrow-free form exists, by Python integers mod r
    otherwise) -> indices that fail"""
    c, W = plan["c"], plan["W"]
    u = D.copy()
    borrow = np.zeros(D.shape[0], dtype=np.int64)
    for w in range(W):
        x = u[:, w] - borrow
        borrow = (x < 0).astype(np.int64)
        u[:, w] = x + (borrow << c)
    ok = (borrow == 0) & (u >= 0).all(axis=1) & (u < (1 << c)).all(axis=1)
    packed, over = pack_windows(np.where(ok[:, None], u, 0), c)
    ok &= ~over & (packed == reduce_mod_r(sc)).all(axis=1)
    bad = []
    for i in np.nonzero(~ok)[0]:
        if sum(int(D[i, w]) << (c * w) for w in range(W)) % R != int.from_bytes(sc[i].tobytes(), "little") % R:
            bad.append(int(i))
    return bad


# ---------------------------------------------------------------- the sort's contract
def keys_and_rows(plan):
    """(set of (scalar index i, window w), row of (i, w)) as functions on arrays, per the header's paragraph"""
    B, mode, n1 = plan["nbuckets"], plan["table_mode"], n_per_vector(plan)

    def set_of(i, w):
        if plan["batch"] > 1:
            return i // n1
        return w if mode == 0 else (np.zeros_like(w) if mode == 1 else w & 1)

    def row_of(i, w):
        if mode == 0:
            return i
        if mode == 1:
            return w * n1 + i % max(n1, 1)
        return (w >> 1) * n1 + i
    return set_of, row_of


def sort_model(D, plan):
    """signed digits int64[n_total, W] -> (offsets uint32[total_buckets + 1], entries uint32[E] in bucket order and sorted
    inside each bucket, bucket of every entry)"""
    set_of, row_of = keys_and_rows(plan)
    i, w = np.nonzero(D)
    d = D[i, w]
    bucket = set_of(i, w) * plan["nbuckets"] + np.abs(d) - 1
    word = (row_of(i, w).astype(np.uint64) | ((d < 0).astype(np.uint64) << np.uint64(31))).astype(np.uint32)
    order = np.lexsort((word, bucket))
    counts = np.bincount(bucket, minlength=plan["total_buckets"])
    assert counts.size == plan["total_buckets"]
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
    return offsets, word[order], bucket[order]


def decode_entries(offsets, entries, plan):
    """what the device wrote -> (scalar index, window, signed digit) of every entry, by the header's paragraph alone"""
    B, mode, n1 = plan["nbuckets"], plan["table_mode"], max(n_per_vector(plan), 1)
    bucket = np.repeat(np.arange(plan["total_buckets"], dtype=np.int64), np.diff(offsets.astype(np.int64)))
    row = (entries & np.uint32(0x7fffffff)).astype(np.int64)
    sign = np.where(entries >> np.uint32(31), -1, 1).astype(np.int64)
    s, mag = bucket // B, bucket % B + 1
    if mode == 0:
        i, w = row, s
    elif mode == 1:
        w, i = row // n1, row % n1 + (s * n1 if plan["batch"] > 1 else 0)
    else:
        w, i = 2 * (row // n1) + s, row % n1
    return i, w, sign * mag, bucket


def items_in_bin_order(D, plan):
    """(key, bin) of the non-zero items in the order the first level sees them (window-major: item w * n + i)"""
    set_of, _ = keys_and_rows(plan)
    w, i = np.nonzero(D.T)
    key = set_of(i, w) * plan["nbuckets"] + np.abs(D[i, w]) - 1
    return key, key >> bin_shift(plan), w * D.shape[0] + i


def facts_of(D, plan):
    offsets, _, _ = sort_model(D, plan)
    runs = np.diff(offsets.astype(np.int64))
    return dict(E=int(offsets[-1]), runs=runs, empty=int((runs == 0).sum()), empty_fraction=float((runs == 0).mean()))


# ---------------------------------------------------------------- families
def _finish(vals, plan, facts=None, below_r=True):
    """window values -> scalars; every scalar of a digit-built family is below r and recodes to exactly its windows"""
    sc, over = pack_windows(vals, plan["c"])
    assert not over.any()
    if below_r:
        assert (vals < plan["nbuckets"]).all() and (vals[:, -1] <= max(top_max(plan), 0)).all()
        assert all(k < R for k in to_ints(sc[:: max(1, len(sc) // 64)])) and np.array_equal(signed_digits(sc, plan), vals)
    f = facts_of(signed_digits(sc, plan), plan)
    f.update(facts or {})
    return sc, f


def _clip_top(vals, plan):
    t = max(top_max(plan), 0)
    vals[:, -1] = np.where(vals[:, -1] <= t, vals[:, -1], 0)
    return vals


def all_zero(plan):
    sc, f = _finish(np.zeros((plan["n"], plan["W"]), dtype=np.int64), plan)
    assert f["E"] == 0
    return sc, f


def uniform(plan, seed=1):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(plan["n"], 32), dtype=np.uint8)
    sc[:, 31] &= 0x1f          # < 2^253 < r
    return sc, facts_of(signed_digits(sc, plan), plan)


def one_bucket(plan, d):
    """every scalar equal.  d = 1, d = B - 1: that digit in every window below the top (one run of n entries per window).
    d = "half": every window below the top holds 2^(c-1): every digit is -2^(c-1) (the last bucket, negated) with a carry
    chain to the top, whose digit is +1."""
    n, W, c, B = plan["n"], plan["W"], plan["c"], plan["nbuckets"]
    vals = np.zeros((n, W), dtype=np.int64)
    if d == "half":
        t = min(W - 1, 252 // c)          # windows that fit below 2^252 < r
        vals[:, :t] = B
        sc, over = pack_windows(vals, c)
        assert not over.any() and all(k < R for k in to_ints(sc[:1]))
        D = signed_digits(sc, plan)
        assert (D[:, 0] == -B).all() and (D[:, 1:t] == -B + 1).all() and (D[:, t] == 1).all() and (D[:, t + 1:] == 0).all()
        f = facts_of(D, plan)
        f["digit_minus_half"] = int((D == -B).sum())
        assert f["digit_minus_half"] == n
        return sc, f
    assert 1 <= d < B
    vals[:, :W - 1] = d
    sc, f = _finish(vals, plan)
    assert f["E"] == n * (W - 1) and set(np.unique(f["runs"])) <= {0, n, n * (W - 1), n * (W // 2), n * ((W - 1) // 2)}
    return sc, f


def minus_half(plan):
    """window 0 holds 2^(c-1), every other window below the top 2^(c-1) - 1: with the carries EVERY digit is -2^(c-1), the one
    digit value the positive families cannot reach (bucket B - 1), in every window, closed by a top digit +1."""
    n, W, c, B = plan["n"], plan["W"], plan["c"], plan["nbuckets"]
    t = min(W - 1, 252 // c)
    vals = np.zeros((n, W), dtype=np.int64)
    vals[:, 0] = B
    vals[:, 1:t] = B - 1
    sc, over = pack_windows(vals, c)
    D = signed_digits(sc, plan)
    assert not over.any() and (D[:, :t] == -B).all() and (D[:, t] == 1).all()
    return sc, facts_of(D, plan)


def staircase(plan, m, wrap=False):
    """window w: point i has digit ((i // m_w) mod (B - 1)) + 1 for i < m_w (B - 1), else 0; m_w cycles through STAIR_M
    starting at m in window 0.  Runs of exactly m_w entries: m = 32 fills whole level-1 chunks, 16 puts two complete runs
    into a chunk, 31 and 33 let the run end drift through every phase of the chunk, 1 ends a run at every entry.
    wrap=True drops the "else 0": the staircase starts over after m_w (B - 1) points, every window of every scalar is non-zero
    (E >= 0.9 max_entries, asserted) and a bucket's run is m_w times the number of turns — the dense form for sizes at which the
    level-1 chunk follows E."""
    n, W, B, n1 = plan["n"], plan["W"], plan["nbuckets"], n_per_vector(plan)
    k0 = STAIR_M.index(m)
    i = np.arange(n, dtype=np.int64) % max(n1, 1)
    vals = np.zeros((n, W), dtype=np.int64)
    ms = [STAIR_M[(k0 + w) % len(STAIR_M)] for w in range(W)]
    for w in range(W):
        vals[:, w] = np.where(wrap | (i < ms[w] * (B - 1)), (i // ms[w]) % (B - 1) + 1, 0)
    sc, f = _finish(_clip_top(vals, plan), plan, dict(ms=ms))
    if wrap:
        assert f["E"] >= 0.9 * plan["max_entries"] and f["E"] >= n * (W - 1)
        if plan["table_mode"] == 0:
            runs = f["runs"].reshape(W, B)
            for w in range(W - 1):          # every bucket of the window: whole steps of m_w, one of them possibly cut by n
                assert runs[w].sum() == n and ((runs[w, :B - 1] % ms[w]) != 0).sum() <= 1 and runs[w, B - 1] == 0
        return sc, f
    if plan["table_mode"] == 0:          # a bucket set per window: the runs are exactly the m_w (the last one cut by n, the top clipped)
        runs = f["runs"].reshape(W, B)
        aligned = []
        for w in range(W - 1):
            full = min(n // ms[w], B - 1)
            assert (runs[w, :full] == ms[w]).all() and runs[w, B - 1] == 0, (w, ms[w])
            start = int(runs[:w].sum())
            if ms[w] == L1_CHUNK and start % L1_CHUNK == 0 and full:
                ends = start + np.cumsum(runs[w, :full])
                edges = np.arange(start + L1_CHUNK, int(ends[-1]) + 1, L1_CHUNK)
                assert np.isin(edges, ends).mean() == 1.0          # every chunk edge of the window is a run end
                aligned.append(w)
        f["chunk_aligned_windows"] = aligned
        if m == L1_CHUNK:
            assert 0 in aligned
    return sc, f


def sparse(plan, stride):
    """only the digits 1, B - 1 and the multiples of `stride` occur (buckets 0, B - 2, stride j - 1), and in the odd windows only the
    multiples: long stretches of empty buckets inside a set, at both ends of the odd sets and across bin borders."""
    n, W, B = plan["n"], plan["W"], plan["nbuckets"]
    if stride >= B:
        raise NotApplicable("stride %d needs more than %d buckets" % (stride, B))
    mult = np.arange(stride, B, stride, dtype=np.int64)
    even = np.unique(np.concatenate(([1, B - 1], mult)))
    rng = np.random.default_rng(stride)
    vals = np.zeros((n, W), dtype=np.int64)
    for w in range(W):
        pool = even if w % 2 == 0 else mult
        vals[:, w] = pool[rng.integers(0, len(pool), size=n)]
    sc, f = _finish(_clip_top(vals, plan), plan)
    assert f["empty_fraction"] >= 0.9, f["empty_fraction"]
    return sc, f


def mostly_zero(plan, p):
    """a fraction p of the scalars is non-zero (all their windows below the top are): p = 0 gives E = 0 (no lane has work, the sum is
    infinity), p = 1/n one scalar (E = its windows), p = 1/64 E << max_entries (most level-1 lanes start beyond E)."""
    n, W, B = plan["n"], plan["W"], plan["nbuckets"]
    rng = np.random.default_rng(7)
    vals = np.zeros((n, W), dtype=np.int64)
    pick = np.zeros(n, dtype=bool)
    if p == "one":
        pick[n // 2] = True
    elif p:
        pick[::int(round(1 / p))] = True
    vals[pick, :W - 1] = rng.integers(1, B, size=(int(pick.sum()), W - 1))
    sc, f = _finish(vals, plan)
    assert f["E"] == int(pick.sum()) * (W - 1)
    if p == 0:
        assert f["E"] == 0
    elif p != "one" and n >= 64:
        assert f["E"] * 32 <= plan["max_entries"]
    return sc, f


def carry_values(plan):
    """the scalars of carry_chain, as integers (any 256-bit values: the device reduces them first)"""
    c, W = plan["c"], plan["W"]
    t = min(W - 1, 252 // c)
    ones = (1 << (c * t)) - 1                                            # digits -1, then zeros with a carry, then +1
    half = sum(((1 << (c - 1)) - (w > 0)) << (c * w) for w in range(t))  # every digit -2^(c-1), then +1
    alt = sum(((1 << (c - 1)) - (w & 1)) << (c * w) for w in range(t))   # 2^(c-1) and 2^(c-1) - 1 in turn: -2^(c-1) twice, then -2^(c-1) + 1 and -2^(c-1)
    top = sum(((1 << c) - 1) << (c * w) for w in range(1, t)) | 1        # +1, then -1 + carries
    base = [R - 1, ones, half, alt, top, 1, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << c) - 1, R - (1 << (c - 1)), (R - 1) // 2]
    return base + [(1 << 256) - 1, R, R + 1, 5 * R + 4] + [R + v for v in base] + [0]


def carry_chain(plan):
    n, c, W, B = plan["n"], plan["c"], plan["W"], plan["nbuckets"]
    vals = carry_values(plan)
    assert all(0 <= v < 1 << 256 for v in vals)
    t = min(W - 1, 252 // c)
    assert signed_digits_int(vals[1], c, W)[:t + 1] == [-1] + [0] * (t - 1) + [1]
    assert signed_digits_int(vals[2], c, W)[:t + 1] == [-B] * t + [1]
    sc = from_ints([vals[i % len(vals)] for i in range(n)])
    D = signed_digits(sc, plan)
    for j in range(min(n, len(vals))):
        assert list(D[j]) == signed_digits_int(vals[j], c, W)
    assert (D[:, -1] >= 0).all() and D.min() >= -B and D.max() < B
    f = facts_of(D, plan)
    f["digit_minus_half"] = int((D == -B).sum())
    if n > 2:
        assert f["digit_minus_half"] >= t          # the all -2^(c-1) value alone gives t of them
    return sc, f


def hot_bin(plan, which=None):
    """several bins: every non-zero digit falls into ONE bin's key range, all other bins stay empty, and a first-level workgroup
    ranks its whole span of 8192 items into that bin.  With a row per second window the weaker fact holds: the two bucket sets take
    turns window by window and a bin of 2048 keys lies inside one set, so at n = 4096 a span is one window of the bin and one window of
    zero digits — the workgroup ranks every non-zero item it has, half a span, into the bin."""
    n, W, B, tb, sh = plan["n"], plan["W"], plan["nbuckets"], plan["total_buckets"], bin_shift(plan)
    nbins = (tb + (1 << sh) - 1) >> sh
    if nbins < 2:
        raise NotApplicable("one bin")
    j = nbins // 2 if which is None else which
    set_of, _ = keys_and_rows(plan)
    rng = np.random.default_rng(j)
    vals = np.zeros((n, W), dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    for w in range(W):
        s = set_of(i, np.full(n, w, dtype=np.int64))
        lo = np.maximum((j << sh) - s * B, 0) + 1                 # digits whose key lies in the bin
        hi = np.minimum(((j + 1) << sh) - s * B, B - 1)
        ok = lo <= hi
        vals[:, w] = np.where(ok, lo + (rng.integers(0, 1 << 30, size=n) % np.maximum(hi - lo + 1, 1)), 0)
    sc, f = _finish(_clip_top(vals, plan), plan)
    key, bins, item = items_in_bin_order(signed_digits(sc, plan), plan)
    assert f["E"] > 0 and (bins == j).all()
    per_span = np.bincount(item // BIN_SPAN)
    # (a row per second window: the two sets take turns window by window, so a span of two windows of 4096 is half zeros)
    assert per_span.max() == (BIN_SPAN if plan["table_mode"] != 2 else BIN_SPAN // 2), "no first-level workgroup with a full span in the bin"
    f["bin"] = j
    return sc, f


TILE_RUN = 4 * STAGE_CAP      # a stretch this long holds a whole staging tile wherever the slices cut and however a span is ordered


def one_key_tile(plan):
    """inside uniform digits, a stretch of >= 4 * STAGE_CAP consecutive items of one bin that carry ONE key: some staging tile of the
    second level ranks all its 8192 entries into one bucket."""
    n, W, B, mode = plan["n"], plan["W"], plan["nbuckets"], plan["table_mode"]
    nw = (TILE_RUN + n - 1) // n if mode == 1 and plan["batch"] == 1 else 1
    if n * nw < TILE_RUN or nw > W - 2:
        raise NotApplicable("no %d consecutive items can share a key" % TILE_RUN)
    rng = np.random.default_rng(5)
    vals = rng.integers(0, B, size=(n, W))
    vals[:, 1:1 + nw] = B // 2 + 1 if B > 2 else 1
    sc, f = _finish(_clip_top(vals, plan), plan)
    key, bins, item = items_in_bin_order(signed_digits(sc, plan), plan)
    k = key[np.searchsorted(item, n)]
    same = (key == k) & (item >= n) & (item < n * (1 + nw))
    assert same.sum() == n * nw >= TILE_RUN
    return sc, f


def all_keys_tile(plan):
    """point i carries digit (i mod 2048) + 1 in every window: the items of bin 0, in the order the second level reads them, carry
    2048 different keys round-robin, so every staging tile holds each key 8192 / 2048 times — the other extreme of the tile's in-LDS
    counting sort.  Needs more than 2048 buckets per set and whole turns of 2048 points."""
    n, W, B = plan["n"], plan["W"], plan["nbuckets"]
    K = 1 << BIN_SHIFT
    if B <= K or n < K or n_per_vector(plan) % K:
        raise NotApplicable("2048 keys round-robin need B > 2048 and n a multiple of 2048")
    vals = np.repeat(((np.arange(n, dtype=np.int64) % n_per_vector(plan)) % K + 1)[:, None], W, axis=1)
    sc, f = _finish(_clip_top(vals, plan), plan, dict(keys_per_tile=K))
    key, bins, item = items_in_bin_order(signed_digits(sc, plan), plan)
    k0 = key[bins == bins[0]]
    assert bins[0] == 0 and k0.size >= TILE_RUN
    stretch = k0[:TILE_RUN]
    assert np.unique(stretch[:K]).size == K and (stretch[K:] == stretch[:-K]).all()      # any 2048 consecutive items: 2048 keys
    return sc, f


FAMILIES = {
    "one_bucket_1": lambda p: one_bucket(p, 1),
    "one_bucket_max": lambda p: one_bucket(p, p["nbuckets"] - 1),
    "one_bucket_half": lambda p: one_bucket(p, "half"),
    "minus_half": minus_half,
    "staircase_1": lambda p: staircase(p, 1),
    "staircase_16": lambda p: staircase(p, 16),
    "staircase_31": lambda p: staircase(p, 31),
    "staircase_32": lambda p: staircase(p, 32),
    "staircase_33": lambda p: staircase(p, 33),
    "staircase_64": lambda p: staircase(p, 64),
    "staircase_160": lambda p: staircase(p, 160),
    "staircase_wrap_32": lambda p: staircase(p, 32, wrap=True),
    "staircase_wrap_33": lambda p: staircase(p, 33, wrap=True),
    "sparse_64": lambda p: sparse(p, 64),
    "sparse_half": lambda p: sparse(p, p["nbuckets"] // 2),
    "mostly_zero_0": lambda p: mostly_zero(p, 0),
    "mostly_zero_one": lambda p: mostly_zero(p, "one"),
    "mostly_zero_64th": lambda p: mostly_zero(p, 1 / 64),
    "carry_chain": carry_chain,
    "hot_bin": hot_bin,
    "one_key_tile": one_key_tile,
    "all_keys_tile": all_keys_tile,
}
SMALL_N_FAMILIES = ("one_bucket_1", "one_bucket_max", "one_bucket_half", "carry_chain")

# the plan shapes of the device tests: (n, window_bits, table_mode)
SORT_SHAPES = [(4096, 0, 0), (1 << 15, 0, 0), (4096, 8, 1), (4096, 13, 1), (4096, 16, 1), (4096, 13, 2)]
SMALL_NS = (1, 2, 63, 65)


def applicable(name, plan):
    """family x plan combinations that exist: decided from the plan alone, so the test lists are fixed at collection"""
    B, n, mode = plan["nbuckets"], plan["n"], plan["table_mode"]
    if name == "sparse_64":
        return B > 64
    if name == "sparse_half":
        return B >= 32          # three digits of B: 90 % of the buckets stay empty from 32 on
    if name == "hot_bin":
        return plan["total_buckets"] > 1 << BIN_SHIFT
    if name == "one_key_tile":
        nw = (TILE_RUN + n - 1) // n if mode == 1 and plan["batch"] == 1 else 1
        return n * nw >= TILE_RUN and nw <= plan["W"] - 2
    if name == "one_bucket_max":
        return B > 2
    if name == "all_keys_tile":
        return B > 1 << BIN_SHIFT and n >= 1 << BIN_SHIFT and n_per_vector(plan) % (1 << BIN_SHIFT) == 0
    return True


def cases(shapes=SORT_SHAPES):
    out = []
    for n, wb, mode in shapes:
        plan = make_plan(n, wb, mode)
        out += [(name, n, wb, mode) for name in FAMILIES if applicable(name, plan)]
    return out


# ---------------------------------------------------------------- base-point patterns for the reductions
def base_logs(pattern, D, plan, seed=11):
    """discrete logs a_i (point i = a_i G) of the n base points -> list of Python integers.
    "random": independent; "equal": all equal to a (with staircase scalars every bucket of a window is m_w P, so the reduction's
    running sum meets an EQUAL addend at its first step: the doubling branch of the general add); "alternating": a for the points
    whose window-0 digit lands in an even bucket, -a for the odd ones (running sums m P, infinity, m P, infinity, ...: the sum
    meets its negative)."""
    import random
    rng = random.Random(seed)
    n = D.shape[0]
    if pattern == "random":
        return [rng.randrange(1, R) for _ in range(n)]
    a = rng.randrange(1, R)
    if pattern == "equal":
        return [a] * n
    assert pattern == "alternating"
    odd = (np.abs(D[:, 0]) - 1) % 2 == 1
    return [R - a if o else a for o in odd]


def expected_log(sc, logs):
    return sum(k * a for k, a in zip(to_ints(reduce_mod_r(sc)), logs)) % R
