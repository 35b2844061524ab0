"""The case table of the 4-channel input builder's stage tests (tests/dtedge_cases.py) reaches every branch of the device's order-statistic
select that an image can reach -- classified from the CPU oracle alone (oracle/dtedge.py), so this runs without a GPU.  The conditions
below are what tests/test_gpu_dtedge_stages.py relies on when it compares the device with the oracle on these same cases."""
import numpy as np
import pytest

import dtedge_cases as dc
from oracle import dtedge as od


@pytest.fixture(scope="module")
def covered():
    out = {}
    for case in dc.CASES:
        for c in dc.categories(case):
            out.setdefault(c, []).append(dc.case_id(case))
    for k in sorted(out):
        print(k, out[k])
    return out


def test_classifier_on_known_keys():
    f = lambda *v: np.array(v, np.float32)
    # 11 values, q = 90: rank 9, successor 10, frac == 0 exactly
    c = dc.classify(f(*([1.0] * 10), 2.0), 90)
    assert (c["rank"], c["succ"], c["source"], c["frac"]) == (9, 10, "top", 0.0)
    # 5 values, q = 90: rank 3, frac 0.6
    assert dc.classify(f(0, 0, 0, 1.0, 1.0), 90)["source"] == "tie"
    one = np.float32(1.0)
    up = lambda k: np.array([one.view(np.uint32) + np.uint32(k)], np.uint32).view(np.float32)[0]
    assert dc.classify(f(0, 0, 0, one, up(1023)), 90)["source"] == "low"       # bits 9..0 differ
    assert dc.classify(f(0, 0, 0, one, up(1024)), 90)["source"] == "mid"       # bit 10
    assert dc.classify(f(0, 0, 0, one, up((1 << 20) - 1)), 90)["source"] == "mid"
    assert dc.classify(f(0, 0, 0, one, up(1 << 20)), 90)["source"] == "top"
    c = dc.classify(f(0, 0, 0, 0, 3.0), 90)
    assert c["key"] == 0 and c["nxt"] == np.float32(3.0).view(np.uint32) and abs(c["frac"] - 0.6) < 1e-12
    assert dc.classify(f(5.0), 99)["succ"] == 0                                  # a single value is its own successor


def test_recipes_are_deterministic_and_small():
    assert len(set(dc.CASES)) == len(dc.CASES)
    for case in dc.CASES:
        a, b = dc.make(case), dc.make(case)
        assert np.array_equal(a, b) and 2 <= case[1] <= 4096 and 2 <= case[2] <= 1024 and a.size <= 3 * 160 * 160, case


def test_stages_agree_with_build_multich():
    for case in dc.CASES[:6]:
        acc, edges, dist, (thr, lo, hi, mn, mx), out = dc.oracle_stages(case)
        img = dc.make(case)
        assert np.array_equal(out, od.build_multich(img, 4))
        assert acc.dtype == np.float32 and dist.dtype == np.float32 and edges.dtype == np.uint8 and set(np.unique(edges)) <= {0, 255}
        assert thr == np.percentile(acc, [od.DT_P_LO, od.DT_P_HI])[1] and (lo, hi) == tuple(np.percentile(dist, [1, 99]))
        assert mn == acc.min() and mx == acc.max() and isinstance(mn, np.float32)
        assert np.array_equal(edges == 255, dist == 0)


@pytest.mark.parametrize("name", ["acc90", "dist99"])
def test_every_successor_source_is_covered(covered, name):
    for s in dc.SOURCES:
        assert "%s:%s" % (name, s) in covered, (name, s)


def test_first_percentile_of_the_distance_has_tie_and_non_tie(covered):
    assert "dist1:tie" in covered
    assert any("dist1:%s" % s in covered for s in ("low", "mid", "top"))


@pytest.mark.parametrize("name", ["acc90", "dist99", "dist1"])
def test_both_lerp_branches_on_a_non_tie(covered, name):
    assert "%s:frac<.5" % name in covered and "%s:frac>=.5" % name in covered


def test_a_case_tells_the_two_lerp_forms_apart(covered):
    """a + d t and b - d (1 - t) usually round to the same float64: at least one case must have t >= 0.5 AND different results, or taking the
    wrong form on the device would go unseen"""
    assert any("%s:lerp-forms-differ" % n in covered for n in ("acc90", "dist99", "dist1"))


def test_edge_conditions_are_covered(covered):
    assert "acc90:frac0" in covered          # frac == 0 with a non-tie successor
    assert any("%s:zero-key" % n in covered for n in ("acc90", "dist99", "dist1"))   # key 0.0, successor non-zero
    assert "no-edge" in covered and "all-edge" in covered and "acc>2^24" in covered
