"""CPU: nmpc_sens_update_batch_multi (csrc/nmpc_sens_multi.hip) as far as it can be held without a GPU.

  - the built gfx950 code object has the twenty instantiations of plan_dirs_kernel<MS>, team sizes 1 .. 10 with and without the per-instance
    field, none with scratch, none with more than 64 KB of LDS; their registers and LDS are printed (DESIGN.md section 5 quotes them);
  - the export and the query are declared, exported and mirrored by nmpc_amd._lib;
  - the inputs of tests/test_gpu_sens_multi.py hold on the numpy reference alone: on every row and point the six directions of
    tests/sens_multi_ref.py give info 0 and 0 < alpha <= 1, and any two of them differ by at least 1000 x the larger of their two bounds, in dw
    — so a kernel that returns direction a in a slot of direction b (emulated here: the reference's directions exchanged) misses the parity
    check by that factor;
  - duality at reference level: the Jacobian the call defines (stage_update with identity dp, column by column) contracted with a cotangent is
    the pbar of tests/sens_adjoint_ref.stage_adjoint, to the two references' own spreads."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sens_adjoint_ref as AR
from tests import sens_multi_ref as MR
from tests import sens_points as SP
from tests import sens_update_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]


def _kernel_notes(tmp_path, name_part):
    """{kernel symbol: {vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size}} of the kernels of lib/libnmpc_hip.so
    whose symbol contains name_part (tests/helpers.kernel_notes, with the LDS)"""
    import importlib
    bld = importlib.import_module("nmpc_amd.build")
    tools = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(tools, "llvm-objcopy")) and os.path.exists(os.path.join(tools, "llvm-readelf"))):
        pytest.skip("no llvm-objcopy / llvm-readelf")
    fat = str(tmp_path / "fat.bin")
    subprocess.check_call([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, bld.SO, str(tmp_path / "copy.so")])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"\x7fELF", data)]
    res = {}
    for n, a in enumerate(starts):
        p = str(tmp_path / ("co%d.elf" % n))
        with open(p, "wb") as f:
            f.write(data[a:starts[n + 1] if n + 1 < len(starts) else len(data)])
        notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", p], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\n\s+\.name:\s+(\S+)", blk)
            if not name or name_part not in name.group(1):
                continue
            res[name.group(1)] = {key: int(re.search(r"\n\s+\.%s:\s+(\d+)" % key, blk).group(1))
                                  for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return res


def test_code_object_has_the_twenty_instantiations_without_scratch_within_64_kb_of_lds(built, tmp_path):
    got = {}
    for name, note in _kernel_notes(tmp_path, "plan_dirs_kernel").items():
        m = re.search(r"^_ZN4nmpc16plan_dirs_kernelILi(\d+)EEE", name)
        assert m, "a kernel of that name with an unknown template signature: " + name
        ms = int(m.group(1))
        got[(ms // 16, ms % 16)] = note
    for (f, m), note in sorted(got.items()):
        print("plan_dirs_kernel m = %2d field %d: %3d registers, %5d bytes of LDS, %d directions per pass" % (
            m, f, note["vgpr_count"], note["group_segment_fixed_size"], 64 - 5 * m))
    assert set(got) == {(f, m) for f in (0, 1) for m in range(1, 11)}, sorted(got)
    for key, note in got.items():
        assert note["private_segment_fixed_size"] == 0, (key, note)
        assert note["group_segment_fixed_size"] <= 65536, (key, note)


def test_export_and_query_are_declared_exported_and_mirrored(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    assert re.search(r"\bint32_t nmpc_sens_update_batch_multi\s*\(", hdr)
    assert re.search(r"#define NMPC_SENS_MAX_DIRS 64\b", hdr) and nmpc_amd._lib.SENS_MAX_DIRS == 64
    q = re.search(r"#define NMPC_QUERY_SENS_DIRS_PER_PASS (\d+)", hdr)
    others = [int(v) for v in re.findall(r"#define NMPC_QUERY_(?!SENS_DIRS_PER_PASS)[A-Z_]+ (\d+)", hdr)]
    assert q and int(q.group(1)) == max(others) + 1 == nmpc_amd._lib.QUERY_SENS_DIRS_PER_PASS      # the next free number
    assert "nmpc_sens_update_batch_multi" in nmpc_amd._lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert any(ln.split()[-1] == "nmpc_sens_update_batch_multi" and " T " in ln for ln in out.splitlines())
    L = nmpc_amd._lib.load()
    assert len(L.nmpc_sens_update_batch_multi.argtypes) == 16
    for name in ("sens_update_multi", "plan_jacobian", "sens_dirs_per_pass"):
        assert hasattr(nmpc_amd.NmpcSolver, name), name
    assert hasattr(nmpc_amd.AdvancedStepController, "correct_scenarios")


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_inputs_hold_on_the_reference_alone(i):
    r = ROWS[i]
    least = np.inf
    for n in range(SP.NPOINTS):
        ref = MR.reference(r, n)
        assert len(ref) == MR.NDIRS
        for d, a in enumerate(ref):
            assert a["info"] == 0 and 0.0 < a["alpha"] <= 1.0, (n, d, a["info"], a["alpha"])
        for a in range(MR.NDIRS):
            for b in range(a + 1, MR.NDIRS):
                # the reference's directions a and b exchanged: what the parity check of slot a would see
                gap = UR.rel(ref[b]["dw"], ref[a]["dw"])
                need = 1000.0 * max(MR.bound(ref[a])[0], MR.bound(ref[b])[0])
                least = min(least, gap / max(MR.bound(ref[a])[0], MR.bound(ref[b])[0]))
                assert gap >= need, (n, a, b, gap, need)
    print("%s: an exchanged pair of directions is at least %.1e bounds away" % (SP.row_id(r), least))


def test_slots_and_d_values():
    assert MR.d_values(14) == [1, 2, 13, 14, 15, 29, 64] and MR.d_values(59) == [1, 2, 58, 59, 60, 64] and MR.d_values(34) == [1, 2, 33, 34, 35, 64]
    for D in (1, 5, 6, 7, 64):
        s = MR.slots(D, 3)
        assert len(s) == D and len(set(s[: MR.NDIRS])) == min(D, MR.NDIRS) and all(s[k] == s[k % MR.NDIRS] for k in range(D))
        assert D < MR.NDIRS or set(s) == set(range(MR.NDIRS))


DUAL_ROWS = [i for i, r in enumerate(ROWS) if r.m in (1, 3, 6, 10)]


@pytest.mark.parametrize("i", DUAL_ROWS, ids=[IDS[i] for i in DUAL_ROWS])
def test_the_jacobian_of_the_stacked_reference_is_the_one_the_adjoint_differentiates(i):
    r = ROWS[i]; cfg = r.cfg
    pt = SP.points(r)[0]
    a = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
    wbar = AR.row_cotangent(r, 0)
    adj = AR.stage_adjoint(*a, wbar)
    sp, _ = AR.spread(*a, wbar)
    n_p = 2 * cfg.nx
    eye = np.eye(n_p)
    J = np.zeros((cfg.n_var, n_p)); tol = np.zeros(n_p)
    for c in range(n_p):
        col = UR.stage_update(*a, dp=eye[c])
        assert col["info"] == 0
        sw, _ = UR.spread(*a, dp=eye[c])
        J[:, c] = col["dw"]
        tol[c] = (100.0 * sw + 1e-12) * np.abs(col["dw"]).max() * np.abs(wbar).sum()
    tol += (100.0 * sp + 1e-12) * np.abs(adj["pbar"]).max()
    err = np.abs(wbar @ J - adj["pbar"])
    print("%s: |wbar' J - pbar| at most %.2e (max|pbar| %.2e), tolerance at least %.2e" % (SP.row_id(r), err.max(), np.abs(adj["pbar"]).max(), tol.min()))
    assert adj["info"] == 0 and (err <= tol).all(), (err.max(), tol.min())
