"""No GPU: the probe of the shared primitives (tests/probes/wave_probe.hip) cross-compiles in both flag sets and probes the project's own
definitions; the references of tests/wave_probe_ref.py hold their own exact cases before tests/test_gpu_wave_probe.py relies on them."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import wave_probe_ref as R


def test_probe_cross_compiles_in_both_flag_sets(tmp_path):
    if R.hipcc() is None:
        pytest.skip("no hipcc on this box")
    for tag, extra in (("fast", []), ("exact", R.EXACT_DEFS)):
        exe = R.compile_probe(tmp_path / ("wave_probe_" + tag), extra)
        assert os.path.getsize(exe) > 0
    cmd = R.probe_command("x")
    assert cmd[1:4] == ["--offload-arch=gfx950", "-O3", "-std=c++17"] or os.environ.get("NMPC_OPT"), cmd


def test_probe_flags_are_the_flags_build_compiles_with(tmp_path, monkeypatch):
    """every compile command of build() starts with the flags codegen_flags() returns, in their order (no compiler runs here)"""
    if R.hipcc() is None:
        pytest.skip("no hipcc on this box")      # build() names the compiler in its commands
    B = R.build_module()
    monkeypatch.setenv("NMPC_EXTRA_DEFS", "-DNMPC_PROBE_FLAG_A=1 -DNMPC_PROBE_FLAG_B=2")
    monkeypatch.setenv("NMPC_OBJDIR", str(tmp_path / "obj"))
    for name, val in (("LIBDIR", str(tmp_path)), ("SO", str(tmp_path / "libnmpc_hip.so")), ("INFO", str(tmp_path / "build_info.json"))):
        monkeypatch.setattr(B, name, val)
    cmds = []
    monkeypatch.setattr(B.subprocess, "check_call", lambda cmd, **kw: cmds.append(list(cmd)))
    B.build(force=True)
    compiles = [c for c in cmds if "-c" in c]
    assert len(compiles) == len(B.UNITS) and len(cmds) == len(compiles) + 1
    want = B.codegen_flags()
    assert want[-2:] == ["-DNMPC_PROBE_FLAG_A=1", "-DNMPC_PROBE_FLAG_B=2"]
    for c in compiles:
        it = iter(c)
        assert all(f in it for f in want), (want, c)      # a subsequence: in the order build() passes them
        other = [f for f in c[1:c.index("-c")] if f not in want]
        # what build() adds beyond them: position-independent code, the source hash (host code), per-source switches named in build.py
        assert all(f == "-fPIC" or f.startswith("-DNMPC_SRC_HASH=") or f.startswith("-DNMPC_COL_") or f in ("-mllvm", "-disable-machine-licm") for f in other), other


def test_probe_includes_the_project_headers_and_defines_no_probed_name():
    src = open(R.PROBE_SRC).read() + open(os.path.join(R.PROBE_DIR, "ipm_cases.h")).read() + open(os.path.join(R.PROBE_DIR, "ipm_cases_host.cpp")).read()
    assert '#include "nmpc_solve_common.h"' in src and '#include "nmpc_ipm.h"' in src
    common = open(os.path.join(R.CSRC, "nmpc_solve_common.h")).read()
    assert all('#include "%s"' % h in common for h in ("nmpc_wave.h", "nmpc_ipm.h", "nmpc_device.h"))
    code = re.sub(r"//[^\n]*", "", src)
    for name in R.PROBED:
        # a definition: the name, a parameter list and a body (or a struct of that name); a call ends in ';' or sits inside an expression
        assert not re.search(r"\b(double|int|bool|void|auto|OptErr)\s+%s\s*\([^;{]*\)\s*(const\s*)?\{" % name, code), name
        assert not re.search(r"\bstruct\s+%s\b" % name, code), name
        assert name == "uniform_f64" or re.search(r"\b%s\b" % name, code), "%s is not probed" % name      # uniform_f64: through every reduction
    assert "__builtin_amdgcn_rcp" in code      # the raw seed is dumped next to the reciprocals
    assert "fma(" not in code and "frexp" not in code      # it restates no formula


def test_fma_model_on_exact_cases():
    f = R.fma
    assert f(0.1, 10.0, -1.0) == float(Fraction(0.1) * 10 - 1) == 2.0 ** -54      # the product's rounding error, which a * b - 1 loses
    assert f(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104      # exact: (1 + e)(1 - e) - 1 = -e^2
    assert f(3.0, 5e-324, 0.0) == 1.5e-323 and f(0.5, 5e-324, 0.0) == 0.0 and f(0.75, 5e-324, 0.0) == 5e-324      # subnormals: exact, tie to even, round up
    assert f(2.0, R.DMAX, 0.0) == math.inf and f(2.0, R.DMAX, -R.DMAX) == R.DMAX      # overflow only of the rounded sum
    assert f(-2.0, R.DMAX, 0.0) == -math.inf
    assert math.isnan(f(math.inf, 0.0, 1.0)) and math.isnan(f(math.inf, 1.0, -math.inf)) and math.isnan(f(1.0, math.nan, 1.0))
    assert f(math.inf, -1.0, 5.0) == -math.inf and f(1.0, 1.0, math.inf) == math.inf
    assert R.bits(f(1.0, -1.0, 1.0)) == R.bits(0.0) and R.bits(f(-0.0, 1.0, -0.0)) == R.bits(-0.0) and R.bits(f(-0.0, 1.0, 0.0)) == R.bits(0.0)
    assert R.bits(f(-1e-200, 1e-200, 0.0)) == R.bits(-0.0)      # an underflow keeps the product's sign
    # 2^53 + 1 is no double: a * b + c with one rounding, where two roundings give another value
    assert f(2.0 ** 27 + 1.0, 2.0 ** 27 - 1.0, 1.0) == 2.0 ** 54 and f(2.0 ** 26, 2.0 ** 27, 1.0) == 2.0 ** 53
    assert f(2.0 ** 26 + 1, 2.0 ** 27, 3.0) == 2.0 ** 53 + 2.0 ** 27 + 4.0      # ... + 3 rounds up to the next even multiple of 2
    rng = np.random.default_rng(1)
    for a, b in rng.standard_normal((500, 2)) * np.exp2(rng.integers(-200, 200, size=(500, 2))):
        a, b = float(a), float(b)
        assert R.mul(a, b) == a * b and f(a, b, 0.0) == a * b and f(a, 1.0, b) == a + b and R.ieee_div(a, b) == a / b
    # one Newton step from an exact seed stays exact; from a seed off by e it lands within e^2 + 2u
    assert R.newton(4.0, 0.25) == 0.25
    r = R.newton(3.0, 0.3333)
    assert R.rel_err_rcp(r, 3.0) <= R.rel_err_rcp(0.3333, 3.0) ** 2 + 2 * R.U
    assert R.ieee_div(1.0, 0.0) == math.inf and R.ieee_div(-1.0, 0.0) == -math.inf and math.isnan(R.ieee_div(0.0, 0.0)) and R.bits(R.ieee_div(1.0, -math.inf)) == R.bits(-0.0)
    assert R.ieee_div(1e-300, 5e-324) == 1e-300 / 5e-324 and R.ieee_div(1.0, 5e-324) == math.inf
    assert R.ulps(1.0, math.nextafter(1.0, 2.0)) == 1 and R.ulps(-5e-324, 5e-324) == 2


def test_butterfly_emulation_against_fsum():
    rng = np.random.default_rng(2)
    for tpb in (64, 128, 256):
        v = np.arange(1.0, tpb + 1.0)      # small integers: every order sums exactly
        assert R.emu_wsum(v) == math.fsum(v) == tpb * (tpb + 1) / 2 and R.emu_wmax(v) == tpb and R.emu_wmin(v) == 1.0
        assert R.emu_wave_min(v) == [1.0 + 64 * w for w in range(tpb // 64)]
        v = rng.standard_normal(tpb) * np.exp2(rng.integers(-30, 31, size=tpb))
        assert abs(R.emu_wsum(v) - math.fsum(v)) <= tpb * R.U * np.abs(v).sum()
        # the order matters and is the butterfly's: lane l adds lane l ^ 32 first
        w = np.zeros(tpb); w[0], w[32], w[1] = 1.0, 2.0 ** -53, 2.0 ** -53
        assert R.emu_wsum(w) == 1.0 and math.fsum(w) == 1.0 + 2.0 ** -52
        w[:] = 0.0; w[0], w[1], w[33] = 1.0, 2.0 ** -53, 2.0 ** -53      # lanes 1 and 33 meet before they reach lane 0
        assert R.emu_wsum(w) == 1.0 + 2.0 ** -52
        v[3] = math.nan
        assert math.isnan(R.emu_wsum(v)) and R.emu_wmax(v) == np.nanmax(v) and R.emu_wmin(v) == np.nanmin(v)
        assert math.isnan(R.emu_wmax(np.full(tpb, math.nan)))


def test_logsum_reference_and_bound():
    import mpmath
    rng = np.random.default_rng(3)
    t = np.exp(rng.uniform(-20.0, 9.0, size=200))
    with mpmath.workprec(200):
        direct = sum(mpmath.log(mpmath.mpf(float(x))) for x in t)
        assert abs(R.ref_logsum(t) - direct) < mpmath.mpf(10) ** -50
        assert abs(R.ref_logsum([5e-324, 2.0 ** 1023]) - (1023 - 1074) * mpmath.log(2)) < mpmath.mpf(10) ** -50
    assert R.logsum_bound(64, 0.5) == 1.1 * 64 * R.U + 4 * R.U


def test_every_edge_class_is_in_the_tables():
    rcp, n_d = R.rcp_table()
    assert 0 < n_d < len(rcp) and len(rcp) < 100000
    d = rcp[:n_d]
    ex = np.frexp(d)[1] - 1
    assert ex.min() == -300 and ex.max() == 300 and (d > 0).any() and (d < 0).any() and np.isfinite(d).all()
    for m in R.SPECIAL_MANT:
        assert (np.abs(d) == math.ldexp(m, -300)).any() and (np.abs(d) == math.ldexp(m, 300)).any()
    full = np.frexp(rcp[n_d:-len(R.EDGE_B)])[1] - 1
    assert set(range(-1022, 1024)) <= set(full.tolist())
    names = [n for n, _ in R.EDGE_B]
    for n in ("0", "min_sub", "max_sub", "2^-1022", "2^1022", "2^1023", "max", "inf"):
        assert "+" + n in names and "-" + n in names
    assert "nan" in names and len(set(names)) == len(names) == 17
    assert {R.fclass(b) for _, b in R.EDGE_B} == {"nan", "+inf", "-inf", "+0", "-0", "finite"}
    assert {R.fclass(a) for _, a in R.EDGE_A} == {"nan", "+inf", "-inf", "+0", "finite"}
    assert [b for _, b in R.EDGE_B][1:3] == [5e-324, math.nextafter(2.0 ** -1022, 0.0)]
    rows, qn_d, edge = R.qdiv_table()
    assert len(rows) - edge == len(R.EDGE_A) * len(R.EDGE_B) and len(rows) + len(rcp) < 100000
    q = np.abs(rows[:qn_d, 0] / rows[:qn_d, 1])
    assert q.min() > 2.0 ** -1000 and q.max() < 2.0 ** 1000      # the accuracy rows: no quotient near the ends of the exponent range
    # LogSum and the reductions: every special in the first and last lane of the first wave, the first lane of the second and the last of the fourth, at every width that has the lane
    planted = {(tpb, sp) for tpb, _, _, sp in R.logsum_cases() if sp}
    for tpb in (64, 128, 256):
        for lane in (0, 63, 64, 255):
            for kind in ("zero", "neg", "nan", "inf"):
                assert ((tpb, (kind, lane)) in planted) == (lane < tpb)
    assert max(t.shape[0] for _, _, t, _ in R.logsum_cases()) == 4096
    assert any((t < 2.0 ** -1022).all() for _, _, t, _ in R.logsum_cases())
    for tpb in (64, 128, 256):
        cs = [v for t, _, v in R.reduce_cases() if t == tpb]
        assert any(np.isnan(v).sum() == 1 for v in cs) and any(np.isnan(v).all() for v in cs) and any((v == math.inf).any() and (v == -math.inf).any() for v in cs)
        assert any((v == 0).all() and np.signbit(v).any() and not np.signbit(v).all() for v in cs)
    pr = R.pair_rows()
    assert sorted(set(pr[:, 0].astype(int))) == list(range(2, 11)) and len(pr) == 2 * sum(m * (m - 1) // 2 for m in range(2, 11))
    br = R.bound_rows()
    assert set(br[:, 0]) == {0.0, 1.0} and set(br[:, 1]) == set(map(float, range(12)))
    # the push's second branch (2 b below max(1, b)) is reached, with values inside, on and beyond the bounds
    assert any(2.0 * s[2] < 1.0 for s in R.BOUND_SETS) and any(s[2] > 1.0 for s in R.BOUND_SETS)
    for vmax, wmax, xymax, thmax in R.BOUND_SETS:
        v = br[br[:, 3] == vmax][:, 2]
        assert (v == xymax).any() and (v == -xymax).any() and (np.abs(v) > max(xymax, thmax)).any() and (v == 0.0).any()
    ir, names = R.ipm_rows()
    assert set(ir[:, 0].astype(int)) == set(range(11)) and ir.shape[1] == R.IPM_IN
    assert set(R.rows_table()[:, 0].astype(int)) == set(range(len(R.R_NAMES))) and set(R.ROW_C) == set(R.R_NAMES)


def test_ipm_rows_walk_the_states_the_rules_give(tmp_path):
    """the rows of the stateful rules carry the state a plain restatement predicts; the host build of the rules must hand back that state"""
    import subprocess
    from tests import test_ipm_control_host as IH
    rows, names = R.ipm_rows()
    exe = tmp_path / "ipm_cases_host"
    subprocess.check_call([IH._compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + R.CSRC, os.path.join(R.PROBE_DIR, "ipm_cases_host.cpp"), "-o", str(exe), "-lm"])
    (tmp_path / "rows.bin").write_bytes(rows.tobytes())
    subprocess.check_call([str(exe), str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")])
    out = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64).reshape(len(rows), R.IPM_OUT)
    for fn, state_in, state_out, n in ((R.MERIT_REF, slice(1, 7), slice(1, 7), 6), (R.LADDER, slice(1, 5), slice(4, 8), 4)):
        idx = [i for i in range(len(rows)) if int(rows[i, 0]) == fn]
        chained = 0
        for a, b in zip(idx, idx[1:]):
            if b == a + 1 and (fn == R.MERIT_REF or max(rows[a, 6], rows[b, 6]) < R.COLD_RETRY_ITERS - 1):      # the cold_retry_due rows stand alone
                assert list(out[a, state_out]) == list(rows[b, state_in]), (names[a], a, out[a], rows[b])
                chained += 1
        assert chained >= 10
    # the values tests/test_ipm_control_host.py holds, through the table form
    merit = [out[i, 0] for i in range(len(rows)) if int(rows[i, 0]) == R.MERIT_REF]
    assert merit == [5.0, 5.0, 5.0, 5.0, 4.0, 4.0, 0.1, 0.1, 0.01, 0.01, 0.001, 0.001]
    shift = [i for i in range(len(rows)) if int(rows[i, 0]) == R.SHIFT]
    for a, b in zip(shift, shift[1:]):
        if rows[a, 3] == rows[b, 3] and rows[b, 2] != 0.0:
            assert out[a, 1] == rows[b, 2]      # shift_next of one row is the delta of the next
    assert sum(out[i, 2] for i in shift) == 2.0      # each schedule ends with its first exhausted shift
    lad = [i for i in range(len(rows)) if int(rows[i, 0]) == R.LADDER]
    acts = [(int(rows[i, 7]), int(rows[i, 6])) for i in lad if out[i, 0] == 1.0 and rows[i, 6] < R.COLD_RETRY_ITERS - 1]
    assert [a for a, _ in acts] == [1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1, 0] and [it for _, it in acts] == [5 * (n + 1) for n in range(12)]
    last = [i for i in lad if rows[i, 6] == 60][0]
    assert list(out[last, 0:3]) == [1.0, 1.0, 0.0]      # stalled, restarts used up, no cold retry left: the solve gives up
