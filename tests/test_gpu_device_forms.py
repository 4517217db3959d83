"""Device-side known answers: the forms the host emulation replaces, run on the GPU one at a time through tests/gpu_kat and compared
with exact integers (Python ints, numpy int64, the oracle's plain C) -- never with the emulation.

  (a) lane primitives: pvq_u3, pvq_isqrt_near, pvq_block_mul / pvq_block_of, mul16x32_q15, smulwb, rot_dot2 + rot_pack, og_add3,
      og_pk_sub_i16, rs_dot2 -- over their whole domain, or a fixed edge set in all combinations plus 4,096 random cases;
  (b) wave_sum, wave_or, wave_scan_add, wave_scan_max: every lane's result;
  (c) the PVQ leaf decode with the whole-wave rotation in the tight layout, over the case lists of tests/test_pvq_kat.py dealt
      into waves in several ways;
  (d) the U table held in registers: every entry, and the ballot search around every entry of every row;
  (e) the wave-uniform inverse-CDF decoder on every SILK table around every threshold, and the lane decoder's packet byte at every
      alignment.
tests/test_device_form_cases.py checks the cases themselves on the CPU.

Measured on an MI355X: pvq_isqrt_near returns the floor minus one at 0 of the 30,977 arguments; pvq_block_mul
returns the larger multiplier at 0 of the 176 block lengths.  The tests print their counts, and the size and a checksum of what
the device returned."""
import math
import zlib

import numpy as np
import pytest

import device_form_cases as dfc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kat():
    return dfc.load_kat()


@pytest.fixture(scope="module")
def prims(kat):
    """Every lane primitive's cases, run once: name -> (inputs, output words [n, 2], expected first word or None)."""
    out = {}
    for name, (entry, rows, want) in dfc.prim_cases().items():
        got = np.zeros((len(rows), dfc.PRIM_OUT), dtype=np.uint32)
        rc = getattr(kat, entry)(rows.ctypes.data, got.ctypes.data, len(rows))
        assert rc == 0, (name, entry, rc)
        print(f"{name}: {len(rows)} cases, device words crc {zlib.crc32(got.tobytes()):08x}")
        out[name] = (rows, got, want)
    return out


def _first(rows, idx, n=5):
    return [rows[i].tolist() for i in idx[:n]]


@pytest.mark.parametrize("name", ["pvq_u3", "pvq_block_of", "mul16x32_q15", "smulwb", "rot_dot2", "rot_pack", "og_add3", "og_pk_sub_i16", "rs_dot2"])
def test_lane_primitive(prims, name):
    rows, got, want = prims[name]
    bad = dfc.mismatches(got[:, 1 if name == "rot_pack" else 0], want)
    assert not bad, (name, len(bad), "first operands:", _first(rows, bad))


def test_pvq_isqrt_near_is_the_floor_or_one_less_at_a_square(prims):
    rows, got, _ = prims["pvq_isqrt_near"]
    bad, low = dfc.isqrt_violations(rows[:, 0], got[:, 0].astype(np.int32))
    squares = [t for t in low if math.isqrt(t) ** 2 == t]
    print(f"pvq_isqrt_near: floor - 1 at {len(low)} of {len(rows)} arguments, {len(squares)} of them perfect squares: {low[:12]}")
    assert not bad, (len(bad), bad[:8])


def test_pvq_block_mul_is_the_floor_plus_one_or_two(prims):
    rows, got, _ = prims["pvq_block_mul"]
    bad, high = dfc.block_mul_violations(rows[:, 0], got[:, 0])
    print(f"pvq_block_mul: the larger M at {len(high)} of {len(rows)} block lengths: {high[:12]}")
    assert not bad, bad
    # ... and pvq_block_of with the device's own M is the division, for every j < 176 (test_lane_primitive[pvq_block_of]): the M
    # it used there is the one returned here
    rows_of, got_of, _ = prims["pvq_block_of"]
    m_of = {int(b): int(m) for b, m in zip(rows_of[:, 1], got_of[:, 1])}
    assert m_of == {int(b): int(m) for b, m in zip(rows[:, 0], got[:, 0])}


@pytest.mark.parametrize("op", ["sum", "or", "scan_add", "scan_max"])
def test_wave_helper_every_lane(kat, op):
    any_v, pos_v = dfc.wave_vectors()
    v = np.ascontiguousarray(pos_v if op == "scan_max" else any_v)
    got = np.zeros_like(v)
    rc = getattr(kat, {"sum": "gk_wave_sum", "or": "gk_wave_or", "scan_add": "gk_wave_scan_add", "scan_max": "gk_wave_scan_max"}[op])(
        v.ctypes.data, got.ctypes.data, len(v))
    assert rc == 0, rc
    print(f"wave {op}: {len(v)} vectors, device words crc {zlib.crc32(got.tobytes()):08x}")
    bad = dfc.mismatches(got, dfc.wave_reference(op, v))
    assert not bad, (op, len(bad), "first (vector, lane):", [(i // 64, i % 64) for i in bad[:8]], v[bad[0] // 64].tolist())


@pytest.fixture(scope="module")
def layout(kat):
    out = np.zeros(5, dtype=np.int32)
    kat.gk_leaf_layout(out.ctypes.data)
    return [int(x) for x in out]


@pytest.fixture(scope="module")
def compositions(layout):
    return dfc.leaf_compositions(layout)


@pytest.mark.parametrize("name", ["order_all_nk", "order_sparse", "shuffled", "rot_lane0_only", "rot_lane63_only", "no_rotation", "many_items"])
def test_pvq_leaves_and_wave_rotation(kat, oracle, layout, compositions, name):
    """pvq_tab_load, pvq_leaf_lane(.., &job) with one leaf per lane, pvq_rotate_wave, as k_celt_recon_fb runs them: every coefficient
    of every wave's spectrum (what lies between the leaves stays zero) and every lane's collapse mask against oc_test_pvq_leaf."""
    ref_coef, ref_mask = dfc.leaf_reference(oracle)
    leaves, place = compositions[name]
    cases, _ = dfc.leaf_lists()
    coef = np.zeros((len(leaves), layout[4]), dtype=np.int16)
    mask = np.zeros((len(leaves), 64), dtype=np.uint32)
    rc = kat.gk_pvq_leaves(leaves.ctypes.data, coef.ctypes.data, mask.ctypes.data, len(leaves))
    assert rc == 0, rc
    print(f"leaves {name}: {len(leaves)} waves, {len(place)} leaves, {int(np.count_nonzero(coef))} non-zero coefficients, "
          f"crc {zlib.crc32(coef.tobytes()):08x} / masks {zlib.crc32(mask.tobytes()):08x}")
    exp, exp_mask, owner = dfc.expected_rows(place, len(leaves), layout[4], ref_coef, ref_mask)
    diff = dfc.compare_leaves(coef, mask, exp, exp_mask, owner, place)
    assert not diff, (name, len(diff), [(d, cases[d[3]] if d[3] >= 0 else None) for d in diff[:6]])


def test_register_u_table_entries_and_search(kat):
    q, want = dfc.utab_queries()
    got = np.zeros(len(q), dtype=np.uint32)
    rc = kat.gk_pvq_tab(q.ctypes.data, got.ctypes.data, len(q))
    assert rc == 0, rc
    print(f"U table: {len(q)} queries, device words crc {zlib.crc32(got.tobytes()):08x}")
    bad = dfc.mismatches(got, want)
    assert not bad, (len(bad), [(q[i].tolist(), int(got[i]), int(want[i])) for i in bad[:8]])


def test_wave_uniform_icdf_around_every_threshold(kat, oracle):
    tabs, subs = dfc.icdf_tables()
    cases = np.ascontiguousarray(dfc.icdf_cases())
    assert kat.gk_rc_icdf_pkt_len() == len(dfc.ICDF_PKT)
    got = np.zeros((len(cases), 6), dtype=np.uint32)
    rc = kat.gk_rc_icdf(tabs, len(tabs), cases.ctypes.data, dfc.ICDF_PKT, got.ctypes.data, len(cases), 8)
    assert rc == 0, rc
    print(f"icdf: {len(subs)} tables, {len(cases)} states, device words crc {zlib.crc32(got.tobytes()):08x}")
    want = dfc.icdf_reference(oracle, tabs, cases, kat.gk_rc_icdf_nbits())
    bad = sorted({i // 6 for i in dfc.mismatches(got, want)})
    names = {off: name for name, off, _ in subs}
    assert not bad, (len(bad), [(names[int(cases[i, 0])], cases[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:6]])


def test_lane_decoder_packet_byte_at_every_alignment(kat):
    n = 40  # three 16-byte pieces at least, whatever the alignment
    data = np.random.default_rng(3).integers(1, 256, n + 63, dtype=np.uint8)  # (no zero: a byte from behind the packet shows)
    got = np.zeros((64, n + 2), dtype=np.uint8)
    rc = kat.gk_rc_lane_bytes(data.ctypes.data, n, got.ctypes.data)
    assert rc == 0, rc
    want = np.zeros_like(got)
    for lane in range(64):
        want[lane, :n] = data[lane:lane + n]
    assert np.array_equal(got, want), [(int(l), int(j), int(got[l, j]), int(want[l, j])) for l, j in np.argwhere(got != want)[:8]]
