"""Build check (no GPU; hipcc cross-compiles): the fused stage-parallel pass of the column kernel leaves its two sweeps as they were.

The pass that computes the optimality error and writes the stage packs sits in the same function as the backward Riccati stage and the
forward sweep, and what the stage-parallel loops keep alive in registers across an iteration is what the sweeps have to work around.  Every
six-robot instantiation — throughput shape and both latency shapes, with and without heading bound and per-instance field — must keep its
backward-stage loop and its forward-sweep loop free of scratch (spill) instructions, and the kernel free of scratch altogether."""
import os
import re
import subprocess
import sys

from tests import test_abi_host as AH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loops(asm, symbol):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_loops.py"), asm, symbol, "--all"], text=True)
    loops = []
    for line in out.splitlines():
        m = re.search(r"loop\s+(\d+)-\s*(\d+):\s+(\d+) instr, dpp\s+(\d+), .*scratch ld\s+(\d+) st\s+(\d+)", line)
        if m:
            loops.append(tuple(int(g) for g in m.groups()))
    return loops, out


def test_sweep_loops_of_every_six_robot_kernel_hold_no_scratch(built, tmp_path):
    asm = AH._col_kernel_asm(tmp_path, 6, also=(2, 10))      # the same three builds test_abi_host.py makes: one hipcc run per session
    kernels = AH._kernel_resources(asm, "solve_col_kernelILi6")
    assert len(kernels) == 12, sorted(kernels)
    for name, res in sorted(kernels.items()):
        loops, out = _loops(asm, name)
        # the innermost loop with the 147 elimination multiply-adds of a row-paired stage, and the one with the 29 of a forward stage
        back = min((lp for lp in loops if lp[3] == 147), key=lambda lp: lp[2])
        fwd = min((lp for lp in loops if lp[3] in (29, 58)), key=lambda lp: lp[2])
        print(name, "backward stage loop", back, "forward loop", fwd, res)
        assert back[4] == 0 and back[5] == 0, (name, out)
        assert fwd[4] == 0 and fwd[5] == 0, (name, out)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0 and res["vgpr_count"] <= 256, (name, res)
