"""CPU checks of the x6 conv tile table (csrc/conv_x6.hip, kTiles) through the two host-only
queries of the built library, which loads without a device: the predicates derived from the
table equal the id ranges they replaced; the table and the chooser's picks are pinned
(tests/golden/conv_x6_tiles.json, conv_x6_plan.json — the plans recorded from the code before
the table existed), so a pull request that adds a tile shows at once whether any other shape's
tile moved.  After a deliberate change of the table or the chooser, re-record both files with
``PYTHONPATH=. python tests/test_conv_x6_tiles.py`` and review the diff."""
import ctypes as C
import json
import os

import pytest

from tcam_wsol_video_amd import _lib
from tcam_wsol_video_amd._lib import tcam_conv_src

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("kind", "bm", "bn", "wm", "wn", "stages", "m16", "il", "lw", "pp", "fp", "group",
          "exact")
THIN = 27
FORMATS = (0, 1, 2, 3)   # x6, f16x3, amp, f16x3 with S3 output


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def num_tiles(lib):
    n = lib.tcam_conv_x6_force_tile(-1)
    assert n == 42
    return n


def tile_info(lib, fmt, tid):
    out = (C.c_int * len(FIELDS))()
    assert lib.tcam_conv_x6_tile_info(fmt, tid, out) == 0
    return dict(zip(FIELDS, out))


def tile_table(lib):
    return {f"{fmt}:{tid}": tile_info(lib, fmt, tid)
            for fmt in FORMATS for tid in range(num_tiles(lib)) if tid != THIN}


def plan(lib, r, sk):
    """The tile id of one record of conv_x6_plan.json under force_streamk(sk)."""
    buf = C.create_string_buffer(32)
    ptr = (C.addressof(buf) + 15) & ~15    # aligned, never read
    arr = (tcam_conv_src * len(r["srcs"]))(*[tcam_conv_src(ptr, *s) for s in r["srcs"]])
    tile = C.c_int(-1)
    lib.tcam_conv_x6_force_streamk(sk)
    try:
        rc = lib.tcam_conv_x6_plan(arr, len(r["srcs"]), r["B"], r["cout"], r["hout"], r["wout"],
                                   *r["k"], *r["pad"], r["fmt"], r["ndst"], r["res"],
                                   C.byref(tile))
    finally:
        lib.tcam_conv_x6_force_streamk(-1)
    return rc, tile.value


# ---- the id ranges the table replaced (the fixed reference of the predicates)
def was_g_tile(i):
    return (10 <= i <= 16) or (22 <= i <= 26) or i >= 28


def was_f16_only_tile(i):
    return i >= 30


def was_m16_tile(i):
    return (14 <= i <= 24) or i == 26 or (28 <= i <= 30) or (34 <= i <= 37) or i >= 39


def was_group_tile(i):
    return i in (15, 26, 17, 18, 20)


def test_predicates_equal_the_id_ranges(lib):
    t = tile_table(lib)
    for tid in range(num_tiles(lib)):
        if tid == THIN:
            continue
        rows = {fmt: t[f"{fmt}:{tid}"] for fmt in FORMATS}
        exact = {fmt: r for fmt, r in rows.items() if r["exact"]}
        assert exact, f"id {tid} is built for no format"
        # an id is LDS-DMA or register-staged in every format, built there or not
        for fmt, r in rows.items():
            assert r["kind"] == was_g_tile(tid), (fmt, tid)
        assert len({r["kind"] for r in rows.values()}) == 1
        assert (0 not in exact) == was_f16_only_tile(tid), tid
        for fmt in (0, 1):
            assert rows[fmt]["group"] == was_group_tile(tid), (fmt, tid)
            # is_m16_tile(fmt, id) reads the row built for fmt; an id that fmt does not build
            # (its fields are then the fallback's) answers from the formats that build it
            own = [exact[fmt]] if fmt in exact else list(exact.values())
            for r in own:
                assert r["m16"] == was_m16_tile(tid), (fmt, tid)


def test_tile_table_is_pinned(lib):
    with open(os.path.join(GOLDEN, "conv_x6_tiles.json")) as f:
        want = json.load(f)
    got = tile_table(lib)
    assert len(got) == 4 * 41
    assert got == want


def test_plans_are_pinned(lib):
    with open(os.path.join(GOLDEN, "conv_x6_plan.json")) as f:
        recs = json.load(f)
    moved = []
    for r in recs:
        for sk in (-1, 0):
            rc, tile = plan(lib, r, sk)
            assert rc == 0, r
            if tile != r["tile"][str(sk)]:
                moved.append((r["name"], r["fmt"], sk, r["tile"][str(sk)], tile))
    assert not moved, f"(shape, fmt, streamk, was, is): {moved}"


def test_plan_file_covers_the_case_tables_and_the_chooser(lib):
    import test_gpu_amp
    import test_gpu_x6
    with open(os.path.join(GOLDEN, "conv_x6_plan.json")) as f:
        recs = json.load(f)
    have = {(r["fmt"], r["B"], json.dumps(r["srcs"]), r["cout"], tuple(r["k"]), r["res"])
            for r in recs}
    for B, srcs, cout, ks, pad, relu, res in test_gpu_x6.X6_CASES:   # test_gpu_f16 runs these too
        for fmt in (0, 1):
            assert (fmt, B, json.dumps([list(s) for s in srcs]), cout, (ks, ks), int(res)) in have
    for srcs, cout, k, pad, relu, res in test_gpu_amp.CONV_CASES:
        s = [[c, h, w, st, u] for (c, h, w, u, st) in srcs]
        assert (2, 2, json.dumps(s), cout, (k, k), int(res)) in have
    # every id the chooser can return without an environment override, in a format that can
    returned = {}
    for r in recs:
        for tile in r["tile"].values():
            returned.setdefault(tile, set()).add(r["fmt"])
    for tid in (2, 3, 6, 15, 17, 18, 20, 23, 26, 27, 30, 31, 35, 36, 41):
        assert tid in returned, tid
    assert any(r["ndst"] == 2 for r in recs)
    assert {r["fmt"] for r in recs} == set(FORMATS)


def test_argument_checks(lib):
    out = (C.c_int * len(FIELDS))()
    for tid in (-1, THIN, 42):
        assert lib.tcam_conv_x6_tile_info(0, tid, out) == -1
    assert lib.tcam_conv_x6_tile_info(4, 0, out) == -1
    ok = dict(name="ok", fmt=0, B=2, srcs=[[64, 14, 14, 1, 0]], cout=64, hout=14, wout=14,
              k=[1, 1], pad=[0, 0], ndst=1, res=0)
    assert plan(lib, ok, -1)[0] == 0
    assert plan(lib, dict(ok, cout=60), -1)[0] == -1                      # Cout % 8 != 0
    assert plan(lib, dict(ok, srcs=[[64, 14, 14, 1, 0]] * 3), -1)[0] == -1  # nsrc == 3
    # a forced tile is honoured like a launch honours it
    lib.tcam_conv_x6_force_tile(5)
    try:
        assert plan(lib, ok, -1) == (0, 5)
    finally:
        lib.tcam_conv_x6_force_tile(-1)


if __name__ == "__main__":   # re-record the golden files from the built library
    L = _lib.load()
    with open(os.path.join(GOLDEN, "conv_x6_tiles.json"), "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v)}'
                                   for k, v in tile_table(L).items()) + "\n}\n")
    with open(os.path.join(GOLDEN, "conv_x6_plan.json")) as f:
        RECS = json.load(f)
    for R in RECS:
        R["tile"] = {str(sk): plan(L, R, sk)[1] for sk in (-1, 0)}
    with open(os.path.join(GOLDEN, "conv_x6_plan.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(R) for R in RECS) + "\n]\n")
