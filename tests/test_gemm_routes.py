"""The route table of the GEMM entry point over a fixed grid of shapes, epilogues, split counts and debug knobs (lcc_debug_gemm_plan: host logic,
no launch, no GPU), compared for equality with the committed record tests/golden/gemm_route_table.json.  The record was taken from the library
BEFORE the dispatch was rewritten as one routing function, so it pins every route of the old dispatch, forced variants included; a deliberate
change of a tile score, predicate or split rule regenerates it (python tests/test_gemm_routes.py) and shows up as a diff of the fixture.
The one switch-dependent case (LCC_GEMM_VH_SMALL=0) is covered by test_gemm_plan.py in a subprocess."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_route_table.json")

MS = [1, 2, 8, 16, 17, 32, 48, 64, 65, 122, 128, 129, 256, 257, 386, 448, 449, 772, 1024, 1131, 1456, 3088, 4096, 4097, 9048, 11648, 24058]
NKS = [[4608, 3584], [3584, 3584], [37888, 3584], [3584, 18944],        # LiveCC-7B: q|k|v, o, gate|up, down
       [3840, 1280], [1280, 1280], [5120, 1280], [1280, 5120],          # vision tower: q|k|v, proj, fc1, fc2
       [2048, 1536], [1536, 1536], [17920, 1536], [1536, 8960],         # Qwen2-VL-2B
       [3584, 3616], [3600, 3584]]                                      # K a multiple of 32 but not of 64; N a multiple of 16 only
EPILOGUES = [0, 1, 2, 3, 4]              # NONE, QUICK_GELU, GELU_ERF, RESIDUAL, SWIGLU (SwiGLU only where N % 32 == 0), each with nsplit = 0
NSPLITS = [1, 3, 4, 6]                   # then EPI_NONE in the split-K slab form
KNOBS = [[2, 64], [3, 64], [4, 64], [7, 64], [8, 64], [13, 64], [14, 64], [15, 64], [2, 16]]      # (gemm variant, skinny rows)
AXES = {"M": MS, "NK": NKS, "epilogues": EPILOGUES, "nsplits": NSPLITS, "knobs": KNOBS}


def cases(n):
    """(epilogue, nsplit) of one shape, in grid order."""
    return [(e, 0) for e in EPILOGUES if e != 4 or n % 32 == 0] + [(0, s) for s in NSPLITS]


def walk(ops):
    """{"tile_rows": one entry per (knobs, M, (N, K), case), "engine_splits": one per (M, (N, K))} of the loaded library."""
    tile_rows, engine_splits = [], []
    try:
        for ki, (variant, rows) in enumerate(KNOBS):
            ops.set_gemm_variant(variant)
            ops.set_skinny_rows(rows)
            for m in MS:
                for n, k in NKS:
                    plans = [ops.gemm_plan(m, n, k, e, nsplit=s) for e, s in cases(n)]
                    tile_rows += [p[0] for p in plans]
                    assert len({p[1] for p in plans}) == 1, (variant, rows, m, n, k)      # a function of the shape alone
                    if ki == 0:
                        engine_splits.append(plans[0][1])
                    else:
                        assert plans[0][1] == engine_splits[(MS.index(m) * len(NKS)) + NKS.index([n, k])], (variant, rows, m, n, k)
    finally:
        ops.set_gemm_variant(ops.GEMM_DEFAULT_VARIANT)
        ops.set_skinny_rows(64)
    return {"tile_rows": tile_rows, "engine_splits": engine_splits}


def regenerate():
    from livecc_amd import ops
    with open(FIXTURE, "w") as f:
        json.dump({"axes": AXES, **walk(ops)}, f, separators=(",", ":"))
        f.write("\n")


def test_every_route_of_the_grid_equals_the_committed_table(built_lib):
    from livecc_amd import ops
    with open(FIXTURE) as f:
        want = json.load(f)
    assert want["axes"] == AXES, "the grid of this file is not the grid the fixture was recorded on"
    got = walk(ops)
    assert len(got["tile_rows"]) == len(want["tile_rows"]) == 30375
    assert got["engine_splits"] == want["engine_splits"]
    if got["tile_rows"] != want["tile_rows"]:
        index = [(kn, m, nk, c) for kn in KNOBS for m in MS for nk in NKS for c in cases(nk[0])]
        moved = [(index[i], want["tile_rows"][i], got["tile_rows"][i]) for i in range(len(index)) if got["tile_rows"][i] != want["tile_rows"][i]]
        pytest.fail(f"{len(moved)} routes moved; the first ((variant, skinny rows), M, (N, K), (epilogue, nsplit)), recorded, now: {moved[:8]}")
    assert set(got["tile_rows"]) == {16, 64, 128, 144, 192, 256, 272, 448}       # every family occurs on the grid


def test_the_plan_is_the_launchs_own_decision(built_lib):
    """What a hand-kept model of the dispatch did not have: the vision q|k|v epilogues (internal codes 6-8) stay on the fixed-height tiles
    where the plain projection of the same shape takes the variable-height ones, and a call gemm_bf16 refuses has no route (0)."""
    from livecc_amd import ops
    try:
        ops.set_gemm_variant(14)         # variable-height tiles wherever legal
        assert ops.gemm_plan(11648, 3840, 1280, ops.EPI_NONE)[0] == 272
        assert [ops.gemm_plan(11648, n, 1280, e)[0] for n, e in ((2560, 6), (1280, 7), (3840, 8))] == [256, 256, 256]
    finally:
        ops.set_gemm_variant(ops.GEMM_DEFAULT_VARIANT)
    assert ops.gemm_plan(11648, 3848, 1280, ops.EPI_NONE)[0] == 0                # N % 16 != 0: LCC_ERR_SHAPE
    assert ops.gemm_plan(386, 3584, 3584, ops.EPI_NONE, nsplit=9)[0] == 0        # more than 8 slabs: LCC_ERR_ARG


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    regenerate()
