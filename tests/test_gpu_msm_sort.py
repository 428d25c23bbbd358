"""GPU: what the MSM sort writes (zk_msm_sort: bucket offsets and entry list, the interface every level-1 kernel consumes)
against its contract, on the adversarial scalar families of tests/msm_distributions.py.  Two checks per case: invariants
read off the device's arrays by the header's paragraph alone (independent of how digits are made), and equality with the
Python model bucket by bucket (order inside a bucket is unspecified: both sides are sorted first)."""
import numpy as np
import pytest

import msm_distributions as md

pytestmark = pytest.mark.gpu


def check_sort(zk, sc, n, wb, mode, batch=1):
    want_plan = md.make_plan(n, wb, mode, batch)
    plan, offsets, entries = zk.msm_sort(sc, n, wb, mode, batch)
    E = plan.pop("entries")
    assert plan == want_plan
    tb = plan["total_buckets"]
    D = md.signed_digits(sc, plan)
    # ---- invariants
    assert offsets.shape == (tb + 1,) and offsets[0] == 0 and offsets[tb] == E == entries.size
    assert (np.diff(offsets.astype(np.int64)) >= 0).all()
    assert E == np.count_nonzero(D) <= plan["max_entries"]
    i, w, d, bucket = md.decode_entries(offsets, entries, plan)
    assert E == 0 or (0 <= i.min() and i.max() < plan["n"] and 0 <= w.min() and w.max() < plan["W"])
    flat = i * plan["W"] + w
    assert np.unique(flat).size == E                                   # every (vector, point, window) at most once
    Ddev = np.zeros_like(D)
    Ddev[i, w] = d
    assert md.digits_value_matches(Ddev, sc, plan) == []               # sum_w d_w 2^(c w) = k mod r for every point
    assert E == 0 or (Ddev[:, -1] >= 0).all()
    # ---- equality with the model
    m_off, m_ent, m_bucket = md.sort_model(D, plan)
    assert np.array_equal(offsets, m_off)
    assert np.array_equal(entries[np.lexsort((entries, bucket))], m_ent)
    return E


@pytest.mark.parametrize("name,n,wb,mode", md.cases())
def test_sort_contract(zk, name, n, wb, mode):
    sc, facts = md.FAMILIES[name](md.make_plan(n, wb, mode))
    assert check_sort(zk, sc, n, wb, mode) == facts["E"]


SMALL_CASES = [(name, n, wb, mode) for wb, mode in [(0, 0), (13, 1)] for n in md.SMALL_NS for name in md.SMALL_N_FAMILIES
               if md.applicable(name, md.make_plan(n, wb, mode))]          # (one_bucket_max with two buckets is one_bucket_1)


@pytest.mark.parametrize("name,n,wb,mode", SMALL_CASES)
def test_sort_contract_small_n(zk, name, n, wb, mode):
    sc, facts = md.FAMILIES[name](md.make_plan(n, wb, mode))
    assert check_sort(zk, sc, n, wb, mode) == facts["E"]


@pytest.mark.parametrize("names", [("staircase_33", "mostly_zero_0", "carry_chain"), ("mostly_zero_0", "one_bucket_half", "sparse_64"),
                                   ("hot_bin_of_one", "uniform", "mostly_zero_0")])
def test_sort_contract_batch_of_three(zk, names):
    """three vectors of 1024 in one sort, a bucket set per vector, a different family in each, one of them all-zero (its
    whole set stays empty between two full ones, or at either end)"""
    n, batch = 1024, 3
    bplan = md.make_plan(n, 0, 1, batch)
    one = md.make_plan(n, bplan["c"], 1)
    assert (one["c"], one["W"]) == (bplan["c"], bplan["W"])
    fam = dict(md.FAMILIES, uniform=lambda p: md.uniform(p), hot_bin_of_one=lambda p: md.one_bucket(p, p["nbuckets"] // 2))
    parts = [fam[name](one) for name in names]
    sc = np.concatenate([p[0] for p in parts])
    E = check_sort(zk, sc, n, 0, 1, batch)
    assert E == sum(p[1]["E"] for p in parts)


def test_sort_uniform_and_scalars_above_r(zk):
    """the ordinary case through the same checks, with raw 256-bit values (reduced on the device first)"""
    rng = np.random.default_rng(3)
    for n, wb, mode in [(5000, 0, 0), (4097, 13, 1), (3001, 12, 2)]:
        sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        check_sort(zk, sc, n, wb, mode)


def test_sort_of_no_scalars(zk):
    """n = 0 (an empty shard in the prover): a full call with no scalars gives E = 0 and all-zero offsets"""
    for wb, mode in [(0, 0), (13, 1)]:
        plan, offsets, entries = zk.msm_sort(b"", 0, wb, mode)
        assert plan["n"] == 0 and plan["entries"] == 0 and entries.size == 0
        assert offsets.shape == (plan["total_buckets"] + 1,) and not offsets.any()
