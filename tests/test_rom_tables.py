"""Generated ROM tables: regeneration is stable, and values equal the reference's literals."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generated_headers_are_up_to_date_and_identical():
    a = open(os.path.join(ROOT, "oracle", "rom_tables.h")).read()
    b = open(os.path.join(ROOT, "esp32-opus-player_amd", "csrc", "rom_tables.h")).read()
    assert a == b
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rom_tables
    assert gen_rom_tables.build_text() == a


def test_tables_equal_reference_literals():
    """Every table with a counterpart in the reference equals its literal there, checked against the value counts and digests
    `tools/check_rom_tables.py --record` took of the reference's tables (tests/golden/rom_reference_tables.json)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_rom_tables as crt
    from silk_rom_data import SILK_TABLES
    with open(os.path.join(ROOT, "tests", "golden", "rom_reference_tables.json")) as fh:
        gold = json.load(fh)
    ours = crt.parse_arrays(open(os.path.join(ROOT, "oracle", "rom_tables.h")).read())
    assert set(gold["pairs"]) == set(crt.PAIRS)
    for name, g in gold["pairs"].items():
        assert (len(ours[name]), crt.digest(ours[name])) == (g["count"], g["sha256"]), name
    known = set(gold["all_tables_sha256"])  # SILK tables keep the reference's order of appearance: matched by content
    for name in SILK_TABLES:
        assert crt.digest(ours[name]) in known, name
    U = ours["rom_pvq_u"]  # dense [15][177]; the reference's rows are ragged
    spans = gold["pvq_u"]["rows"]
    assert len(spans) == 15
    assert crt.digest([U[n * 177 + k] for n, k0, k1 in spans for k in range(k0, k1)]) == gold["pvq_u"]["sha256"]
