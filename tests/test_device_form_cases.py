"""The cases of tests/test_gpu_device_forms.py, checked on the CPU: the GPU test cannot pass by being empty or lopsided, every case
lies inside the domain the drivers' host wrappers accept, and the comparators report a reference that differs in one place."""
import numpy as np
import pytest

import device_form_cases as dfc


@pytest.fixture(scope="module")
def kat():
    return dfc.load_kat()


@pytest.fixture(scope="module")
def layout(kat):
    out = np.zeros(5, dtype=np.int32)
    kat.gk_leaf_layout(out.ctypes.data)
    return [int(x) for x in out]


@pytest.fixture(scope="module")
def compositions(layout):
    return dfc.leaf_compositions(layout)


def test_leaf_lists_are_the_cpu_tests_lists():
    cases, n_first = dfc.leaf_lists()
    assert n_first > 20000 and len(cases) - n_first > 10000  # the thresholds of tests/test_pvq_kat.py
    assert {c[3] for c in cases[:n_first]} == {1, 2, 4, 8, 16} and {c[5] for c in cases[:n_first]} == {0, 1, 2, 3}
    assert max(c[0] for c in cases) == 176 and min(c[0] for c in cases) == 2


def test_layout_keeps_clear_of_the_table_rows_in_the_tops(layout):
    lo0, hi0, lo1, hi1, row = layout
    assert 0 <= lo0 < hi0 <= lo1 < hi1 == row
    assert hi0 - lo0 == 800 and hi1 - lo1 == 800  # eband[21] = 100 bins of 8: what bands reach of a channel's 960 coefficients


def test_wave_compositions_hold_each_named_kind(compositions):
    cases, _ = dfc.leaf_lists()
    seen = set()
    for name, (leaves, place) in compositions.items():
        seen.update(ci for _, _, _, ci in place)
        assert len({(w, lane) for w, lane, _, _ in place}) == len(place)
        tot = dfc.wave_item_totals(place, len(leaves))
        if name == "rot_lane0_only":
            assert len(tot) >= dfc.N_DIRECTED and all(t[3] == [0] for t in tot)
        if name == "rot_lane63_only":
            assert len(tot) >= dfc.N_DIRECTED and all(t[3] == [63] for t in tot)
        if name == "no_rotation":
            assert len(tot) >= dfc.N_DIRECTED and all(t[0] == 0 for t in tot)
            assert all((leaves[w, :, 7] == 1).all() for w in range(len(leaves)))  # full waves that return early
        if name == "many_items":
            assert sum(1 for t in tot if t[1] > 64 and t[2] > 64) >= 16  # the `base` loop runs more than once in both passes
        if name == "shuffled":  # rotated and unrotated leaves share waves
            assert sum(1 for w, t in enumerate(tot) if 0 < t[0] < (leaves[w, :, 7] == 1).sum()) > len(tot) // 2
    assert seen == set(range(len(cases)))  # every case of both lists runs
    everything = [t for leaves, place in compositions.values() for t in dfc.wave_item_totals(place, len(leaves))]
    assert sum(1 for t in everything if t[1] > 64) >= 16 and sum(1 for t in everything if t[2] > 64) >= 16


def test_every_leaf_case_passes_the_wrappers_domain_check(kat, compositions, layout):
    for name, (leaves, place) in compositions.items():
        assert leaves.dtype == np.uint32 and leaves.flags.c_contiguous
        assert kat.gk_pvq_leaves_check(leaves.ctypes.data, len(leaves)) == 0, name
    # ... and the check is one: a leaf across the first channel's top, an index outside the codebook, two leaves on one coefficient
    leaves = compositions["many_items"][0][:1].copy()
    assert kat.gk_pvq_leaves_check(leaves.ctypes.data, 1) == 0
    for lane, word, value in ((0, 3, layout[1] - 1), (0, 2, 0xFFFFFFFF), (1, 3, int(leaves[0, 0, 3])), (0, 4, 3), (0, 0, 177)):
        bad = leaves.copy()
        bad[0, lane, word] = value
        assert kat.gk_pvq_leaves_check(bad.ctypes.data, 1) == -1, (lane, word, value)


def test_every_other_case_lies_in_its_form_s_domain():
    prims = dfc.prim_cases()
    assert len(prims["pvq_u3"][1]) == 2047 and len(prims["pvq_isqrt_near"][1]) == 176 * 176 + 1 and len(prims["pvq_block_mul"][1]) == 176
    assert len(prims["pvq_block_of"][1]) == 176 * 176
    for name in ("mul16x32_q15", "smulwb", "rot_dot2", "og_add3", "og_pk_sub_i16", "rs_dot2"):
        assert len(prims[name][1]) >= dfc.N_RANDOM + 25 and len(prims[name][1]) == len(prims[name][2])
    a, b, c, d, e = -32768 & dfc.M32, -32768 & dfc.M32, -32768 & dfc.M32, -32768 & dfc.M32, 16384
    at = [i for i, r in enumerate(prims["rot_dot2"][1].tolist()) if r == [a, b, c, d, e]]
    assert at and prims["rot_dot2"][2][at[0]] == ((-(1 << 31) + 16384) >> 15) & dfc.M32  # 2^31 + 16384 wrapped, not clamped
    any_v, pos_v = dfc.wave_vectors()
    assert any_v.shape[1] == 64 and pos_v.shape[1] == 64 and (pos_v >= 0).all() and len(pos_v) >= 64 + 256
    assert (np.abs(any_v.astype(np.int64).sum(axis=1)) >= 1 << 31).sum() >= 2  # sums that wrap 32 bits
    q, want = dfc.utab_queries()
    assert len(q) == len(want) and (q[:, 0] == 0).sum() >= 16 * 192 and (q[:, 0] == 1).sum() > 3 * 14 * 15
    assert set(q[q[:, 0] == 1][:, 1].tolist()) == set(range(1, 15))
    tabs, subs = dfc.icdf_tables()
    assert len({name for name, _, _ in subs}) == len(dfc.ICDF_TABLES) and all(off + 64 <= len(tabs) for _, off, _ in subs)
    assert all(e[-1] == 0 and 0 not in e[:-1] and len(e) <= 42 for _, _, e in subs)
    cases = dfc.icdf_cases()
    assert len(cases) > 5 * 3 * len(subs) and set(cases[:, 1].tolist()) == set(dfc.ICDF_RNGS)
    assert (cases[:, 2] < cases[:, 1]).all() and set(cases[:, 0].tolist()) == {off for _, off, _ in subs}


def test_comparators_report_one_altered_value(oracle, compositions, layout):
    ref_coef, ref_mask = dfc.leaf_reference(oracle)
    leaves, place = compositions["many_items"]
    exp, exp_mask, owner = dfc.expected_rows(place, len(leaves), layout[4], ref_coef, ref_mask)
    assert dfc.compare_leaves(exp, exp_mask, exp, exp_mask, owner, place) == []
    w, lane, pos, ci = place[5]
    coef, mask = exp.copy(), exp_mask.copy()
    coef[w, pos + 3] += 1
    mask[w, lane] ^= 1 << 7
    assert dfc.compare_leaves(coef, mask, exp, exp_mask, owner, place) == [("coef", w, pos + 3, ci), ("mask", w, lane, ci)]
    stray = exp.copy()  # a store where no leaf lies
    free = np.argwhere(owner == -1)[0]
    stray[free[0], free[1]] = 1
    assert dfc.compare_leaves(stray, exp_mask, exp, exp_mask, owner, place) == [("coef", int(free[0]), int(free[1]), -1)]
    # one lane of one scan
    _, pos_v = dfc.wave_vectors()
    want = dfc.wave_reference("scan_max", pos_v)
    got = want.copy()
    got[17, 48] += 1
    assert dfc.mismatches(want, want) == [] and dfc.mismatches(got, want) == [17 * 64 + 48]
    # one root: the floor minus one where the argument is no perfect square, and the floor plus one
    tq = np.arange(176 * 176 + 1)
    r = np.array([int(np.sqrt(t)) for t in tq])
    assert dfc.isqrt_violations(tq, r) == ([], [])
    r[50] -= 1
    r[49] -= 1
    r[64] += 1
    assert dfc.isqrt_violations(tq, r) == ([50, 64], [49, 50])
    blen = np.arange(1, 177)
    m = 65536 // blen + 1
    m[2] += 1
    m[9] += 2
    assert dfc.block_mul_violations(blen, m) == ([10], [3])
