"""A.w / B.w over rows of any length (csrc/fieldops.hip): rows above the cut are summed chunk by chunk,
a wave each, and the values — so the proofs — are byte for byte those of the lane-per-row kernel.  Expected values come from
Python integers, the committed goldens, the C restatement (oracle/c_oracle.py) or the toxic waste, never from the library's
other path alone.  ZKHIP_SPMV_ROW_CUT is read at every create and operator call: 0 = no row is long, n = rows above n terms."""
import functools

import numpy as np
import pytest

from conftest import CIRCUITS, golden_bytes, golden_json, golden_path
from oracle import bn254 as bn, c_oracle as co

pytestmark = pytest.mark.gpu

G1B = bn.g1_to_bytes(bn.G1.gen)
G2B = bn.g2_to_bytes(bn.G2.gen)
CUTS = {"default": None, "cut1": "1", "cut0": "0"}


def _set_cut(monkeypatch, cut):
    if CUTS[cut] is None:
        monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_SPMV_ROW_CUT", CUTS[cut])


@functools.lru_cache(maxsize=None)
def _builtin_cut():
    """the built-in T: what a prover reports when the variable is not set (the caller has unset it)"""
    import rapidsnark_old_amd as zk
    p = zk.Prover(golden_path("multiplier2", "circuit.zkey"))
    cut = p.info()["spmv_row_cut"]
    p.close()
    return cut


# ---------------------------------------------------------------- 1. the operator, exact at every cut point
N_ROWS, N_VARS = 64, 40


def _lengths(T):
    return [0, 1, 7, 8, 9, T - 1, T, T + 1, 63, 64, 65, 254, 1023, 1024, 1025, 2049, 4096, 70000]


@functools.lru_cache(maxsize=None)
def _operator_case(where, values, T):
    """-> (image, nCoefs, witness, want_a, want_b): one row of each length of _lengths in matrix A, in B, or at the same row
    index in both; the other rows 0 to 3 terms.  Records permuted, signals out of 40 (every long row reuses them)."""
    from rapidsnark_old_amd import synth
    rng = np.random.default_rng(sum(map(ord, where + values)) + T)
    lens = _lengths(T)
    rows_of = rng.permutation(N_ROWS)[:len(lens)]
    count = rng.integers(0, 4, size=(2, N_ROWS))
    for mat in (0, 1):
        if where in ("AB"[mat], "both"):
            count[mat, rows_of] = lens
    m_col = np.repeat([0, 1], count.sum(axis=1)).astype(np.uint32)
    c_col = np.concatenate([np.repeat(np.arange(N_ROWS), count[mat]) for mat in (0, 1)]).astype(np.uint32)
    nnz = c_col.size
    rec = np.zeros(nnz, dtype=synth.COEF_DTYPE)
    rec["m"], rec["c"], rec["s"] = m_col, c_col, rng.integers(0, N_VARS, size=nnz, dtype=np.uint32)
    top = np.frombuffer((bn.R_MOD - 1).to_bytes(32, "little"), dtype=np.uint8)
    rec["v"] = np.tile(top, (nnz, 1)) if values == "r_minus_1" else synth.random_fr_bytes(rng, nnz).reshape(-1, 32)
    rec = rec[rng.permutation(nnz)]
    if values == "r_minus_1":
        w = np.tile(top, N_VARS)
    elif values == "above_r":                       # 256-bit words in [r, 2^256): summed as the words they are
        w = np.frombuffer(b"".join(int(bn.R_MOD + int(x)).to_bytes(32, "little") for x in rng.integers(0, 1 << 62, size=N_VARS)), dtype=np.uint8)
        w = w.copy()
        w[31::32] |= 0xC0
    else:
        w = synth.random_fr_bytes(rng, N_VARS).reshape(-1).copy()
    img = np.empty(4 + nnz * 44, dtype=np.uint8)
    img[:4] = np.frombuffer(np.uint32(nnz).tobytes(), dtype=np.uint8)
    img[4:] = rec.view(np.uint8).reshape(-1)
    wi = [int.from_bytes(w[32 * i:32 * i + 32].tobytes(), "little") for i in range(N_VARS)]
    want = [[0] * N_ROWS, [0] * N_ROWS]
    vals = [int.from_bytes(v.tobytes(), "little") for v in rec["v"]]
    rinv = pow(1 << 256, -1, bn.R_MOD)
    for mat, row, sig, v in zip(rec["m"].tolist(), rec["c"].tolist(), rec["s"].tolist(), vals):
        want[mat][row] += wi[sig] * v
    want = [[x * rinv % bn.R_MOD for x in side] for side in want]              # sum of w * v / R: the reference's Montgomery products
    return img, nnz, w, want[0], want[1]


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("values", ["random", "r_minus_1", "above_r"])
@pytest.mark.parametrize("where", ["A", "B", "both"])
def test_operator_exact_at_every_cut_point(zk, monkeypatch, where, values, cut):
    """zk_fr_coef_accumulate on a 64-row domain, nVars = 40: rows of 0 ... 70000 terms around every length at which the sums
    change path (the cut T, a lane's 16 terms, a chunk's 1024, several chunks, more partials than a wave has lanes), against
    big-int sums; coefficients and witness at r - 1 (the lazy sums' extreme) and witness words above r."""
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    img, nnz, w, want_a, want_b = _operator_case(where, values, _builtin_cut())
    assert bn.mont_mul(5, 7, bn.R_MOD) == 35 * pow(1 << 256, -1, bn.R_MOD) % bn.R_MOD      # (the form `want` is in)
    _set_cut(monkeypatch, cut)
    a, b = zk.fr_coef_accumulate(img, nnz, N_ROWS, w)
    got_a = [int.from_bytes(a[32 * i:32 * i + 32].tobytes(), "little") for i in range(N_ROWS)]
    got_b = [int.from_bytes(b[32 * i:32 * i + 32].tobytes(), "little") for i in range(N_ROWS)]
    assert got_a == want_a and got_b == want_b


# ---------------------------------------------------------------- 2. every golden on the new path
@pytest.mark.parametrize("name", CIRCUITS)
def test_goldens_on_the_long_row_path(zk, monkeypatch, name):
    """With the cut at 1 every row of two or more terms is a long row: the golden proof bytes, and the counts the prover
    reports against the key's own records.  (multiplier2 is a * b = c: none of its four records shares a row with another, so
    no cut makes a long row in it — its 0 is checked like the other keys' 9 ... 390; the other four must and do report > 0.)"""
    from rapidsnark_old_amd import synth
    meta = golden_json(name, "meta.json")
    wt = golden_bytes(name, "witness.wtns")
    data = golden_bytes(name, "circuit.zkey")
    start, nbytes = zk.open_existing(data, "zkey", 1).sections[4][0]
    rec = np.frombuffer(data[start + 4:start + nbytes], dtype=synth.COEF_DTYPE)
    terms = np.unique(rec["m"].astype(np.int64) << 32 | rec["c"], return_counts=True)[1]
    want_long = int((terms > 1).sum())
    assert want_long > 0 or name == "multiplier2"
    monkeypatch.setenv("ZKHIP_SPMV_ROW_CUT", "1")
    p = zk.Prover(golden_path(name, "circuit.zkey"))
    info = p.info()
    assert info["spmv_row_cut"] == 1 and info["spmv_longest_row"] == terms.max()
    assert info["spmv_long_rows"] == want_long and info["spmv_chunks"] == want_long          # (every row is one chunk)
    assert p.prove(wt, r=int(meta["r"]), s=int(meta["s"])).hex() == meta["proof_bytes"]
    p.close()
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT")
    p = zk.Prover(golden_path(name, "circuit.zkey"))
    info = p.info()
    assert info["spmv_chunks"] == 0 and info["spmv_long_rows"] == 0 and info["spmv_row_cut"] >= 16
    assert p.prove(wt, r=int(meta["r"]), s=int(meta["s"])).hex() == meta["proof_bytes"]
    p.close()


# ---------------------------------------------------------------- 3. whole proofs against the C restatement
K = 8
LONG_A = (9, 64, 254, 4097)         # rows 1, 2, 3, 4 of A
LONG_B = 70000                      # row 5 of B only: every long row lies in the first block of a chain cut in 2 or 4
R_S = (0x1357924680ACE, (1 << 200) + 99)


@functools.lru_cache(maxsize=None)
def _pool():
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth
    mk = lambda k: synth.workload(k, zk.synth_chain_g1, zk.synth_chain_g2, zk.g1_mul, zk.g2_mul, synth.g1_gen_bytes(), synth.g2_gen_bytes())
    return mk(K), mk(K + 2)


@functools.lru_cache(maxsize=None)
def _long_key(n_vars, n_public):
    """The irregular-shape key of test_gpu_synth.py at k = 8 (nVars != domainSize, tables cut from a larger pool) plus the
    records of the long rows -> (workload, witnesses, C-restatement view)."""
    from rapidsnark_old_amd import synth
    n = 1 << K
    small, big = _pool()
    wl = dict(small)
    wl["nVars"], wl["nPublic"] = n_vars, n_public
    for name, width in (("pointsA", 64), ("pointsB1", 64), ("pointsB2", 128)):
        wl[name] = np.ascontiguousarray(np.asarray(big[name]).reshape(-1)[: n_vars * width])
    wl["pointsC"] = np.ascontiguousarray(np.asarray(big["pointsC"]).reshape(-1)[: (n_vars - n_public - 1) * 64])
    rec = np.asarray(wl["coefs"])[4:].view(synth.COEF_DTYPE).copy()
    rng = np.random.default_rng(K * 1000 + n_vars)
    rec["s"] = np.where(rec["s"] < n_vars, rec["s"], rec["s"] % n_vars) if n_vars <= n else rng.integers(0, n_vars, size=rec.shape[0], dtype=np.uint32)
    extra = []
    for mat, row, terms in [(0, 1 + i, t) for i, t in enumerate(LONG_A)] + [(1, 5, LONG_B)]:
        have = int(((rec["m"] == mat) & (rec["c"] == row)).sum())
        x = np.zeros(terms - have, dtype=synth.COEF_DTYPE)
        x["m"], x["c"], x["s"] = mat, row, rng.integers(0, n_vars, size=x.size, dtype=np.uint32)
        x["v"] = synth.random_fr_bytes(rng, x.size).reshape(-1, 32)
        extra.append(x)
    rec = np.concatenate([rec] + extra)
    rec = rec[rng.permutation(rec.size)]
    img = np.empty(4 + rec.size * 44, dtype=np.uint8)
    img[:4] = np.frombuffer(np.uint32(rec.size).tobytes(), dtype=np.uint8)
    img[4:] = rec.view(np.uint8).reshape(-1)
    wl["coefs"], wl["nCoefs"] = img, int(rec.size)
    ws = []
    for _ in range(4):
        w = synth.random_fr_bytes(rng, n_vars).reshape(-1).copy()
        w[:32] = np.frombuffer((1).to_bytes(32, "little"), dtype=np.uint8)
        ws.append(w)
    return wl, ws, co.ZkeyView(wl)


@functools.lru_cache(maxsize=None)
def _want(n_vars, n_public, i, r=R_S[0], s=R_S[1]):
    wl, ws, view = _long_key(n_vars, n_public)
    return co.prove(view, ws[i], r, s)


def _long_rows_and_chunks(T):
    long = [t for t in LONG_A + (LONG_B,) if t > T]
    return len(long), sum((t + 1023) // 1024 for t in long)


def _prover(zk, wl, **kw):
    from rapidsnark_old_amd import views
    return views.ProverFromView(zk, wl, device=0, shard_index=kw.get("shard_index", 0), shard_count=kw.get("shard_count", 1), window_bits=0,
                                timings=False, precomp=kw.get("precomp", False), partitioned_chain=kw.get("partitioned_chain", False),
                                batch=kw.get("batch", 0))


def _destroy(p):
    import ctypes as C
    p.lib.zk_prover_destroy(p.h)
    p.h = C.c_void_p()


SHAPES = [(200, 0), (300, 5)]


@pytest.mark.parametrize("precomp", [False, True, 2])
@pytest.mark.parametrize("n_vars,n_public", SHAPES)
def test_long_row_key_bit_exact_vs_c_oracle(zk, monkeypatch, n_vars, n_public, precomp):
    """Rows of 9, 64, 254 and 4097 terms in A and one of 70000 in B only: the five MSM sums and the proof against the C
    restatement, in the three table modes."""
    import torch
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl, ws, view = _long_key(n_vars, n_public)
    p = _prover(zk, wl, precomp=precomp)
    info = p.info()
    T = info["spmv_row_cut"]
    assert info["spmv_longest_row"] == LONG_B and (info["spmv_long_rows"], info["spmv_chunks"]) == _long_rows_and_chunks(T)
    wd = torch.from_numpy(ws[0]).to("cuda:0")
    assert p.prove_msm_dev(wd.data_ptr()) == co.prove_msm(view, ws[0])
    assert p.prove_dev(wd.data_ptr(), *R_S) == _want(n_vars, n_public, 0)
    _destroy(p)


# ---------------------------------------------------------------- 4. the other ways in
@pytest.mark.parametrize("count", [1, 3, 4])
def test_batch_prover_on_the_long_row_key(zk, monkeypatch, count):
    """opts.batch = 4: `count` witnesses share the chunk descriptors, each has its own partial sums"""
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl, ws, _ = _long_key(*SHAPES[1])
    p = _prover(zk, wl, precomp=True, batch=4)
    assert p.info()["spmv_chunks"] > 0
    rs = [(R_S[0] + i, R_S[1] + 3 * i) for i in range(count)]
    p.submit_batch(ws[:count], rs)
    assert p.collect_batch(count) == [_want(*SHAPES[1], i, *rs[i]) for i in range(count)]
    _destroy(p)


def test_four_proofs_in_flight_on_the_long_row_key(zk, monkeypatch):
    """submit / collect after reserve(4): the partial sums belong to the proof slot"""
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl, ws, _ = _long_key(*SHAPES[0])
    p = _prover(zk, wl)
    p.reserve(4)
    for w in ws:
        p.submit_host(w, *R_S)
    assert [p.collect() for _ in ws] == [_want(*SHAPES[0], i) for i in range(4)]
    _destroy(p)


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_provers_on_the_long_row_key(zk, monkeypatch, shards):
    import torch
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl, ws, _ = _long_key(*SHAPES[1])
    wd = torch.from_numpy(ws[1]).to("cuda:0")
    provers = [_prover(zk, wl, shard_index=i, shard_count=shards, precomp=(i % 2 == 1)) for i in range(shards)]
    assert all(q.info()["spmv_chunks"] > 0 for q in provers)            # (every shard of an unpartitioned chain computes every row)
    parts = [q.prove_msm_dev(wd.data_ptr()) for q in provers]
    assert provers[0].prove_finish(parts, *R_S) == _want(*SHAPES[1], 1)
    for q in provers:
        _destroy(q)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_partitioned_chain_on_the_long_row_key(zk, monkeypatch, devices):
    """A chain partitioned over shards of one device: the long rows are among rows 1 to 4 of A and row 5 of B, all in shard
    0's block — that shard runs the long-row path, the others the lane-per-row kernel alone."""
    from rapidsnark_old_amd import views
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl, ws, _ = _long_key(*SHAPES[0])
    mp = views.MultiProverFromView(zk, wl, devices)
    assert mp.chain_partitioned and mp.n_shards == len(devices)
    infos = [mp.shard_info(i) for i in range(mp.n_shards)]
    assert (infos[0]["spmv_long_rows"], infos[0]["spmv_chunks"]) == _long_rows_and_chunks(infos[0]["spmv_row_cut"]) and infos[0]["spmv_longest_row"] == LONG_B
    assert all(x["spmv_long_rows"] == 0 and x["spmv_chunks"] == 0 and x["spmv_longest_row"] < 16 for x in infos[1:])
    assert mp.prove(ws[2], *R_S) == _want(*SHAPES[0], 2)
    mp.close()


# ---------------------------------------------------------------- 5. a valid key with long rows
def test_zkgen_long_rows_key_is_valid(zk, monkeypatch, tmp_path):
    """zkgen.generate(long_rows=...): the proof equals the toxic-waste prediction and the C restatement's, the pairing check
    accepts it, and the .r1cs written for the key describes the same circuit."""
    from rapidsnark_old_amd import zkgen, views
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    k, npub = 10, 2
    key = zkgen.generate(k, npub, seed=3, long_rows=[(1, 5000), (4, 300)])
    rec = np.asarray(key["coefs"])[4:].view(zkgen.synth.COEF_DTYPE)
    per_row = np.bincount(rec["m"].astype(np.int64) * (1 << k) + rec["c"], minlength=2 << k)
    assert sorted(per_row[per_row > 3].tolist()) == [300, 300, 300, 300, 5000]
    assert (per_row[:1 << k] > 3).sum() == 3 and (per_row[1 << k:] > 3).sum() == 2            # A: picks 0, 2, 4; B: picks 1, 3
    assert ((per_row[:1 << k] > 3) & (per_row[1 << k:] > 3)).sum() == 2                        # two constraints are long on both sides
    pairs = rec["m"].astype(np.int64) << 40 | rec["c"].astype(np.int64) << 20 | rec["s"]
    assert np.unique(pairs).size < pairs.size                                                  # (row, signal) pairs repeat
    r, s = 0x13579BDF, (1 << 247) - 99
    a, b, c = zkgen.expected_proof_dlogs(key, r, s)
    want = zk.g1_mul(G1B, a) + zk.g2_mul(G2B, b) + zk.g1_mul(G1B, c)
    p = views.ProverFromView(zk, key, device=0, shard_index=0, shard_count=1, window_bits=0, timings=False)
    info = p.info()
    assert info["spmv_longest_row"] >= 5000 and info["spmv_long_rows"] == 5 and info["spmv_chunks"] == 5 + 4
    proof = p.prove_host(key["witness"], r, s)
    _destroy(p)
    assert proof == want
    assert co.prove(co.ZkeyView(key), key["witness"], r, s) == want
    zkgen.write_all(key, str(tmp_path))
    zkgen.write_r1cs(key, str(tmp_path / "circuit.r1cs"))
    public = np.asarray(key["witness"])[32:32 * (1 + npub)].tobytes()
    with zk.VerificationKey.from_json(str(tmp_path / "verification_key.json")) as vk:
        assert vk.verify(proof, public).tolist() == [0]
    rc = zk.R1cs(str(tmp_path / "circuit.r1cs"))
    assert rc.check(np.ascontiguousarray(key["witness"])).ok
    assert rc.match_zkey(str(tmp_path / "circuit.zkey")) == (0, None)
    rc.close()


def test_zkgen_long_rows_compose_with_circuit_like(zk, monkeypatch):
    """circuit_like's second layer needs two passes for the witness; the extended sides read input signals only, so the
    passes still close: the proof equals the toxic-waste prediction and the C restatement's."""
    from rapidsnark_old_amd import zkgen, views
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    key = zkgen.generate(10, 2, seed=4, circuit_like=True, long_rows=[(2, 300)])
    assert key["nVars"] == 3 * 1024 // 4 + 5
    r, s = 0x2468ACE, (1 << 230) + 17
    a, b, c = zkgen.expected_proof_dlogs(key, r, s)
    want = zk.g1_mul(G1B, a) + zk.g2_mul(G2B, b) + zk.g1_mul(G1B, c)
    p = views.ProverFromView(zk, key, device=0, shard_index=0, shard_count=1, window_bits=0, timings=False)
    info = p.info()
    assert info["spmv_long_rows"] == 2 and info["spmv_longest_row"] == 300 and info["spmv_chunks"] == 2
    proof = p.prove_host(key["witness"], r, s)
    _destroy(p)
    assert proof == want == co.prove(co.ZkeyView(key), key["witness"], r, s)


def test_zkgen_without_long_rows_is_unchanged(zk):
    from rapidsnark_old_amd import zkgen
    a, b = zkgen.generate(10, 2, seed=3), zkgen.generate(10, 2, seed=3, long_rows=())
    for name in ("coefs", "pointsA", "pointsB1", "pointsB2", "pointsC", "pointsH", "pointsIC", "witness"):
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name
    assert a["trap"]["toxic"] == b["trap"]["toxic"]


# ---------------------------------------------------------------- 6. the record check still holds
@pytest.mark.parametrize("field,value", [("c", 1 << K), ("s", 300)])
def test_record_out_of_range_in_a_long_row_key_is_a_create_error(zk, monkeypatch, field, value):
    from rapidsnark_old_amd import synth
    monkeypatch.delenv("ZKHIP_SPMV_ROW_CUT", raising=False)
    wl = dict(_long_key(*SHAPES[1])[0])
    img = np.asarray(wl["coefs"]).copy()
    rec = img[4:].view(synth.COEF_DTYPE)
    at = int(np.nonzero((rec["m"] == 1) & (rec["c"] == 5))[0][100])            # a term of the 70000-term row
    rec[field][at] = value
    wl["coefs"] = img
    with pytest.raises(zk.ZkHipError, match="out of range"):
        _prover(zk, wl)
