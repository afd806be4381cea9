"""Reader of tests/golden/gemm_plan.txt, the recorded plans of the GEMM launcher ("<shape> -> <plan>" lines, tests/test_gemm_plan_cpu.py),
shared by that test and by the GPU test that runs the tile the file names (tests/test_bench_shapes_gpu.py)."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.txt")

# the recorded tile names -> the switch that forces that tile (astts_op_gemm_set_ring_mode / ASTTS_GEMM_RING)
MODE_OF_TILE = {"128x128": 1, "128x64": 2, "64x64": 3, "256x256-1barrier": 4, "256x256-8phase": 5}


def lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def ring_tile(m, n, k, mode=-1, blockmax=False):
    """The ring tile recorded for a plain fp16 GEMM [m, k] x [n, k] (aligned x, fp32 out) under ring switch `mode`: the "ring" line of
    the shape lists "switch:tile" for the switches -1 .. 5 (a kernel kind such as T128 where the ring kernels do not run)."""
    key = f"ring m={m} n={n} k={k} bm={int(blockmax)} ->"
    found = [ln[len(key):].split() for ln in lines() if ln.startswith(key)]
    assert len(found) == 1, (key, found)
    return dict(tok.split(":") for tok in found[0])[str(mode)]
