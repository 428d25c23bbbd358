"""CPU: the Python model of the MSM sort's contract (tests/msm_distributions.py) against the library's plan-only
zk_msm_sort, the digit restatement against plain integers, and every family's self-assertions at the shapes the device tests
use — a family whose scalars lack the property it is named for fails HERE, not silently on the GPU."""
import random

import numpy as np
import pytest

import msm_distributions as md

NS = [1, 2, 63, 64, 65, 1 << 10, 1 << 12, 1 << 15, 1 << 17, 1 << 19, 1 << 20, 1 << 21, 1 << 22]
WBITS = [0, 2, 3, 8, 13, 15, 16, 17, 20, 22]


@pytest.mark.parametrize("mode,batch", [(0, 1), (1, 1), (2, 1), (1, 2), (1, 8)])
def test_plan_restatement_matches_the_library(zk, mode, batch):
    for n in NS:
        for wb in WBITS:
            try:
                want = md.make_plan(n, wb, mode, batch)
            except ValueError:
                with pytest.raises(zk.ZkHipError):
                    zk.msm_sort(None, n, wb, mode, batch, plan_only=True)
                continue
            got, offsets, entries = zk.msm_sort(None, n, wb, mode, batch, plan_only=True)
            assert offsets is None and entries is None
            assert got.pop("entries") == 0
            assert got == want, (n, wb, mode, batch)
            c, W = want["c"], want["W"]
            assert W * c >= 255 and (W - 1) * c < 256 and want["nbuckets"] == 1 << (c - 1)
            assert (md.R >> ((W - 1) * c)) + 1 < 1 << (c - 1) or W * c >= 256          # the top digit cannot go negative


def test_plan_refusals(zk):
    for args in [(1024, 0, 3, 1), (1024, 0, 0, 2), (1024, 0, 2, 4), (1 << 27, 8, 0, 1), (1 << 24, 13, 1, 16), (1 << 31, 0, 0, 1)]:
        with pytest.raises(ValueError):
            md.make_plan(*args)
        with pytest.raises(zk.ZkHipError):
            zk.msm_sort(None, *args, plan_only=True)
    # the largest n * W that is accepted, and the first that is not (plain tables, W = 16 at c = 16)
    assert md.make_plan((1 << 28) - 1, 16)["max_entries"] < 1 << 32
    assert zk.msm_sort(None, (1 << 28) - 1, 16, plan_only=True)[0]["max_entries"] == ((1 << 28) - 1) * 16
    with pytest.raises(ValueError):
        md.make_plan(1 << 28, 16)
    with pytest.raises(zk.ZkHipError):
        zk.msm_sort(None, 1 << 28, 16, plan_only=True)
    # table rows: W * n < 2^31 with a row per window
    with pytest.raises(ValueError):
        md.make_plan(1 << 27, 16, 1)
    with pytest.raises(zk.ZkHipError):
        zk.msm_sort(None, 1 << 27, 16, 1, plan_only=True)


def test_argument_checks_that_come_before_any_device_use(zk):
    from rapidsnark_old_amd import lib as L
    import ctypes as C
    plan = L.zk_msm_sort_plan()
    plan.size = C.sizeof(plan)
    off = np.zeros(8, dtype=np.uint32)
    assert L.load_library().zk_msm_sort(None, 4, 0, 0, 1, C.byref(plan), off.ctypes.data, None) != 0      # one array only
    plan.size = 0
    assert L.load_library().zk_msm_sort(None, 4, 0, 0, 1, C.byref(plan), None, None) != 0                 # size not set


@pytest.mark.parametrize("c", [2, 3, 6, 8, 9, 13, 15, 16, 17, 20, 22])
def test_digit_restatement(c):
    plan = md.make_plan(1 << 12, c, 1)
    assert plan["c"] == c
    W = plan["W"]
    rng = random.Random(c)
    ks = [rng.getrandbits(256) for _ in range(10000 // 11 + 1)] + md.carry_values(plan) + [md.R - 1, md.R, 0, 1, (1 << 256) - 1]
    D = md.signed_digits(md.from_ints(ks), plan)
    for k, row in zip(ks, D):
        ref = md.signed_digits_int(k, c, W)
        assert list(row) == ref
        assert sum(d << (c * w) for w, d in enumerate(ref)) == k % md.R
        assert all(-(1 << (c - 1)) <= d < 1 << (c - 1) for d in ref) and ref[-1] >= 0
    assert md.digits_value_matches(D, md.from_ints(ks), plan) == []
    D2 = D.copy()
    D2[3, 1] += 1
    assert md.digits_value_matches(D2, md.from_ints(ks), plan) == [3]


def test_digit_restatement_random_values_at_the_plain_plans():
    """10^4 random 256-bit values through the windows the direct MSMs use (c = 6, 9, 13)"""
    rng = random.Random(1)
    ks = [rng.getrandbits(256) for _ in range(10000)]
    sc = md.from_ints(ks)
    for n in (4096, 1 << 15, 1 << 19):
        plan = md.make_plan(n)
        D = md.signed_digits(sc, plan)
        B = plan["nbuckets"]
        assert D.min() >= -B and D.max() < B and (D[:, -1] >= 0).all()
        assert md.digits_value_matches(D, sc, plan) == []
        for j in range(0, 10000, 97):
            assert list(D[j]) == md.signed_digits_int(ks[j], plan["c"], plan["W"])


def test_model_round_trip():
    """decode_entries inverts sort_model in every table mode (and with a batch): the two halves of the device test agree"""
    for n, wb, mode, batch in [(300, 0, 0, 1), (300, 8, 1, 1), (300, 7, 2, 1), (100, 8, 1, 3)]:
        plan = md.make_plan(n, wb, mode, batch)
        sc, _ = md.uniform(plan)
        D = md.signed_digits(sc, plan)
        offsets, entries, bucket = md.sort_model(D, plan)
        i, w, d, b2 = md.decode_entries(offsets, entries, plan)
        assert np.array_equal(bucket, b2)
        D2 = np.zeros_like(D)
        D2[i, w] = d
        assert np.array_equal(D, D2) and offsets[-1] == np.count_nonzero(D)


@pytest.mark.parametrize("name,n,wb,mode", md.cases())
def test_family_self_assertions(name, n, wb, mode):
    plan = md.make_plan(n, wb, mode)
    sc, facts = md.FAMILIES[name](plan)
    assert sc.shape == (n, 32) and sc.dtype == np.uint8
    assert facts["E"] <= plan["max_entries"]
    if name.startswith("sparse"):
        assert facts["empty_fraction"] >= 0.9
    if name == "all_keys_tile":
        assert plan["c"] >= 13 and facts["keys_per_tile"] == 2048
    if name == "staircase_32" and mode == 0:
        assert facts["chunk_aligned_windows"]


@pytest.mark.parametrize("n", md.SMALL_NS)
@pytest.mark.parametrize("name", md.SMALL_N_FAMILIES)
def test_family_self_assertions_small_n(name, n):
    for wb, mode in [(0, 0), (13, 1)]:
        plan = md.make_plan(n, wb, mode)
        if md.applicable(name, plan):
            md.FAMILIES[name](plan)


# every (shape, family) the sum tests and the prover tests run that the sort shapes above do not cover
SUM_SHAPES = [(2048, 0, 0)] + [(1 << k, wb, mode) for k in (10, 12) for wb, mode in [(0, 0), (0, 1), (13, 1), (18, 1), (13, 2)]]


@pytest.mark.parametrize("n,wb,mode", SUM_SHAPES)
def test_family_self_assertions_at_the_sum_tests_shapes(n, wb, mode):
    plan = md.make_plan(n, wb, mode)
    for name in md.FAMILIES:
        if md.applicable(name, plan):
            md.FAMILIES[name](plan)


@pytest.mark.parametrize("name,n", [(name, 1 << 17) for name in ("one_bucket_1", "one_bucket_max", "one_bucket_half")]
                         + [(name, 1 << 19) for name in ("staircase_wrap_32", "staircase_wrap_33", "one_bucket_1")])
def test_family_self_assertions_at_the_large_sizes(name, n):
    plan = md.make_plan(n)
    sc, facts = md.FAMILIES[name](plan)
    if n == 1 << 19:
        assert facts["E"] > 32 * md.ROUND_LANES_MAX          # the level-1 chunk follows E whatever the occupancy


def test_families_that_cannot_exist_say_so():
    with pytest.raises(md.NotApplicable):
        md.hot_bin(md.make_plan(4096))
    with pytest.raises(md.NotApplicable):
        md.one_key_tile(md.make_plan(4096))
    with pytest.raises(md.NotApplicable):
        md.sparse(md.make_plan(4096), 64)
    with pytest.raises(md.NotApplicable):
        md.all_keys_tile(md.make_plan(4096, 8, 1))
    with pytest.raises(md.NotApplicable):
        md.all_keys_tile(md.make_plan(1024, 13, 1))
