"""The cells of the construction walks (build_search_kernel, refine_search_kernel, add_link_kernel: <METRIC, BS, PREC>) that
tests/test_gpu_add_beams.py and tests/test_gpu_build_beams.py walk, one table for the three kernels: four (metric, precision) pairs,
and per pair the efConstruction values that put the beam into two register slots (up to 128), four (up to 256) or LDS (up to 512),
the boundaries on both sides.

Shapes: 48 columns, m = 4 (mMax0 = 8: lists fill and prune at once, the upper layers are populated), clustered rows, levels forced by
test_gpu_add.draw_levels' law with m = 4; 1600 rows where the beam is in LDS, 800 below.

Soft-deleted nodes: a case asks for a number (a tenth of its start graph, or the 60 of test_add_with_deleted_nodes) and gets at most
rows - 3 * efConstruction, so that the live rows at level 0 stay at 3 * efConstruction and a full beam goes on evicting: with 800 rows
at efConstruction 256 that leaves 32, with 1600 rows at 512 it leaves 64 -- 4 % instead of 10 % in those two columns."""
import functools
import os
import subprocess
import tempfile

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
DIM, M = 48, 4

EDGES = (128, 129, 256, 257, 512)
CELLS = ([("f32-l2", L2, F32, e) for e in EDGES] + [("i8-cos", COSINE, I8, e) for e in EDGES] +
         [("f32-cos", COSINE, F32, e) for e in (200, 300)] + [("f16-l2", L2, F16, e) for e in (200, 300)])
CELL_IDS = [f"{name}-{efc}" for name, _, _, efc in CELLS]
assert len(CELLS) == 14

# efConstruction -> the BS a walk kernel must be instantiated with (0: the LDS beam).  Written down from KDB_WALK_KERNEL's rule as
# the cases were designed, NOT computed from the code under test: walk_bs() below reads what the code does
WANT_BS = {128: 2, 129: 4, 200: 4, 256: 4, 257: 0, 300: 0, 512: 0}
UP_MARK_CAP = 256           # KDB_UP_MARK_CAP: an upper layer walked with ef above it can mark more than the un-mark list holds
# The un-mark list really overflows only where a walk of an upper layer REACHES more than 256 nodes.  With m = 4 it never does: on
# these corpora (and on uniform rows) the level-1 graph the oracle builds falls into islands, the entry point's holds 44 to 90 of the
# roughly 410 nodes of level >= 1, whatever share of the rows is raised (measured: 411, 781, 1181 upper nodes -> 44, 61, 44 reached).
# So each kernel gets "up" cases beside its cells: m = 8 and every second node raised (level law with base 2), where the level-1 walk
# of efConstruction 512 hands back 512 candidates and level 2 still reaches about 300
UP_M, UP_LEVEL_BASE = 8, 2
UP_CELLS = [("f32-l2", L2, F32, 512), ("i8-cos", COSINE, I8, 512)]
UP_IDS = [f"{name}-{efc}-up" for name, _, _, efc in UP_CELLS]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_for(efc):
    return 1600 if efc >= 257 else 800


def dead_for(n, efc, asked):
    return max(0, min(asked, n - 3 * efc))


@functools.lru_cache(maxsize=None)
def walk_bs(efcs):
    """kdb_walk_bs for each efConstruction of the tuple, from kdb_walk_lds.h itself through tests/cpp/walk_plan_test.cpp (the
    program of tests/test_walk_plan.py, in its `bs` mode)"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "walk_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "kektordb_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "walk_plan_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
        r = subprocess.run([exe, "bs"] + [str(e) for e in efcs], check=True, capture_output=True, text=True, timeout=60)
    out = tuple(int(x) for x in r.stdout.split())
    assert len(out) == len(efcs), r.stdout
    return dict(zip(efcs, out))


def assert_walk_bs(efc):
    """the case runs the beam storage it was written for"""
    got = walk_bs(tuple(sorted(WANT_BS)))
    assert got[efc] == WANT_BS[efc], (efc, got)


def reached(graph, level, start):
    """nodes a walk from `start` can reach on `level` of an exported graph (oracle.Graph), itself included"""
    off, nb = graph.offsets[level], graph.neighbors[level]
    seen, stack = {int(start)}, [int(start)]
    while stack:
        x = stack.pop()
        for y in nb[int(off[x]):int(off[x + 1])].tolist():
            if y not in seen:
                seen.add(y)
                stack.append(y)
    return len(seen)
