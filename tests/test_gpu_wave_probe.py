"""GPU: the arithmetic and wave primitives every solve kernel shares, each held on its own against an exact reference.

tests/probes/wave_probe.hip includes csrc/nmpc_solve_common.h (and through it nmpc_wave.h, nmpc_ipm.h) and applies each primitive to the
tables of tests/wave_probe_ref.py; it is built twice with the library's code-generation flags — as the library is built, and with
-DNMPC_FAST_DIV=0 -DNMPC_RCP_STEPS=2 — and each binary runs once, as a child process.  One test per group; the figures each one prints are
the ones docs/WAVE_PRIMITIVES.md quotes."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import test_ipm_control_host as IH
from tests import wave_probe_ref as R

pytestmark = pytest.mark.gpu
U = R.U
DOC = os.path.join(R.ROOT, "docs", "WAVE_PRIMITIVES.md")


def run_probe(exe, tables, dump):
    """one run of a probe binary as a child process; a non-zero exit or a timeout fails the module"""
    try:
        r = subprocess.run([exe, str(tables), str(dump)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("%s did not finish in 120 s" % exe, pytrace=False)
    if r.returncode != 0:
        pytest.fail("%s: exit status %d\n%s" % (exe, r.returncode, r.stderr[-2000:]), pytrace=False)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if R.hipcc() is None:
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("wave_probe")
    sections, info = R.all_sections()
    R.write_tables(d / "tables.bin", sections)
    out = {"info": info, "sections": sections}
    for tag, extra in (("fast", []), ("exact", R.EXACT_DEFS)):      # the second binary is not started when the first one failed
        exe = R.compile_probe(d / ("wave_probe_" + tag), extra)
        run_probe(exe, d / "tables.bin", d / (tag + ".bin"))
        out[tag] = R.read_dump(d / (tag + ".bin"), sections)
    return out


# ---------------------------------------------------------------- the checks: plain functions of (dump, info), so a saved dump can be read again
def seed_error(dump, info):
    """e0: the largest relative error of the dumped v_rcp_f64 seed over the working domain D"""
    k, vals, n_d = info["rcp"]
    seed = R.as_f64(dump[k][:, 0])
    return max(R.rel_err_rcp(float(seed[i]), float(vals[i])) for i in range(n_d))


def check_reciprocals(dump, info, exact):
    k, vals, n_d = info["rcp"]
    w = R.as_f64(dump[k])
    kq, rows, qn_d, edge = info["qdiv"]
    wq = R.as_f64(dump[kq])
    # bit-exact model: from the dumped seed every Newton step is two IEEE fmas, on every input, specials included
    for i in range(len(vals)):
        d, seed = float(vals[i]), float(w[i, 0])
        r1 = R.newton(d, seed)
        r2 = R.newton(d, r1)
        assert R.same(float(w[i, 1]), r1), ("rcp1", d, seed, float(w[i, 1]), r1)
        assert R.same(float(w[i, 2]), r2), ("rcp2", d, seed, float(w[i, 2]), r2)
        assert R.same(float(w[i, 3]), r2 if exact else r1), ("rcp_nr", d, seed, float(w[i, 3]))
    for i in range(len(rows)):
        a, b, seed = float(rows[i, 0]), float(rows[i, 1]), float(wq[i, 0])
        want = R.ieee_div(a, b) if exact else R.mul(a, R.newton(b, seed))
        assert R.same(float(wq[i, 1]), want), ("qdiv", a, b, seed, float(wq[i, 1]), want)
    # accuracy over D against the exact quotient
    e0 = seed_error(dump, info)
    assert e0 <= 2.0 ** -22, "the v_rcp_f64 seed is worse than 2^-22 (%.3e): the bounds below mean nothing" % e0
    fig = {"e0": e0}
    fig["rcp1"] = max(R.rel_err_rcp(float(w[i, 1]), float(vals[i])) for i in range(n_d))
    fig["rcp2"] = max(R.rel_err_rcp(float(w[i, 2]), float(vals[i])) for i in range(n_d))
    fig["rcp_nr"] = max(R.rel_err_rcp(float(w[i, 3]), float(vals[i])) for i in range(n_d))
    fig["qdiv"] = max(R.rel_err_div(float(wq[i, 1]), float(rows[i, 0]), float(rows[i, 1])) for i in range(qn_d))
    fig["rcp_nr ulps"] = max(R.ulps(float(w[i, 3]), R.ieee_div(1.0, float(vals[i]))) for i in range(n_d))
    print("reciprocals (%s build): " % ("exact" if exact else "product") + ", ".join("%s %.4g" % kv for kv in fig.items())
          + "; bounds e0^2 + 2u = %.4g, 2u = %.4g, e0^2 + 3u = %.4g" % (e0 * e0 + 2 * U, 2 * U, e0 * e0 + 3 * U))
    assert fig["rcp1"] <= e0 * e0 + 2 * U
    assert fig["rcp2"] <= 2 * U
    if exact:
        assert fig["rcp_nr ulps"] <= 1 and fig["rcp_nr"] <= 2 * U
    else:
        assert fig["rcp_nr"] <= e0 * e0 + 2 * U
        assert fig["qdiv"] <= e0 * e0 + 3 * U
    return fig


def edge_divergence(dump, info):
    kq, rows, qn_d, edge = info["qdiv"]
    wq = R.as_f64(dump[kq])
    e0 = seed_error(dump, info)
    return R.divergence(lambda k: float(wq[edge + k, 1]), e0 * e0 + 3 * U)


def edge_table(dump, info):
    """lines 'b: seed, rcp1, rcp2, rcp_nr' with the class of each (a finite one with its relative error against 1 / b)"""
    k, vals, n_d = info["rcp"]
    w = R.as_f64(dump[k])
    lines = []
    for j, (name, b) in enumerate(R.EDGE_B):
        i = len(vals) - len(R.EDGE_B) + j
        assert R.same(float(vals[i]), b)

        def cls(x):
            c = R.fclass(x)
            return c if c != "finite" or b == 0.0 or math.isinf(b) else "finite (%.2g)" % R.rel_err_rcp(x, b)
        lines.append("%s: seed %s, rcp1 %s, rcp2 %s, rcp_nr %s, IEEE 1/b %s" % (name, cls(float(w[i, 0])), cls(float(w[i, 1])), cls(float(w[i, 2])), cls(float(w[i, 3])),
                                                                              R.fclass(R.ieee_div(1.0, b))))
    return lines


def documented(marker):
    """the lines of the fenced block that follows '<!-- marker -->' in docs/WAVE_PRIMITIVES.md"""
    text = open(DOC).read()
    at = text.index("<!-- %s -->" % marker)
    body = text[at:].split("```")[1]
    return [ln.strip() for ln in body.strip().splitlines() if ln.strip()]


def check_logsum(dump, info):
    import mpmath
    worst = {"wlogsum": 0.0, "wave_logsum": 0.0}
    for k, cases in info["logsum"]:
        w = R.as_f64(dump[k])      # [case][5][lane]
        for ci, (tpb, name, terms, special) in enumerate(cases):
            got, gotw = w[ci, 0], w[ci, 1]
            tag = "%s, %d threads" % (name, tpb)
            assert len({R.bits(float(x)) for x in got if x == x}) <= 1 and (np.isnan(got).all() or not np.isnan(got).any()), ("lanes differ", tag)
            nwave = tpb // 64
            for wv in range(nwave):
                lanes = gotw[64 * wv:64 * wv + 64]
                assert len({R.bits(float(x)) for x in lanes if x == x}) <= 1 and (np.isnan(lanes).all() or not np.isnan(lanes).any()), ("lanes differ", tag, wv)
            if special is not None:
                kind, lane = special
                hit = lane // 64
                if kind == "inf":      # log(+inf) = +inf: the sum is +inf, as the logarithm's would be
                    assert got[0] == math.inf, (tag, got[0])
                    assert gotw[64 * hit] == math.inf, (tag, gotw[64 * hit])
                else:                  # a term <= 0 or NaN makes the result NaN, as the header promises
                    assert math.isnan(got[0]), (tag, got[0])
                    assert math.isnan(gotw[64 * hit]), (tag, gotw[64 * hit])
                others = [wv for wv in range(nwave) if wv != hit]
            else:
                others = list(range(nwave))
            refs = {wv: R.ref_logsum(terms[:, 64 * wv:64 * wv + 64]) for wv in others}
            for wv in others:      # the LIDAR kernel's form, per wave
                ref = refs[wv]
                err = float(abs(mpmath.mpf(float(gotw[64 * wv])) - ref))
                bound = R.logsum_bound(terms.shape[0] * 64, float(ref))
                worst["wave_logsum"] = max(worst["wave_logsum"], err / bound)
                assert err <= bound, ("wave_logsum", tag, wv, float(gotw[64 * wv]), float(ref), err, bound)
            if special is None:
                assert all(r > 0 for r in refs.values()) or all(r < 0 for r in refs.values()), ("the bound's premise: wave sums of one sign", tag)
                ref = sum(refs.values())
                err = float(abs(mpmath.mpf(float(got[0])) - ref))
                bound = R.logsum_bound(terms.size, float(ref))
                worst["wlogsum"] = max(worst["wlogsum"], err / bound)
                assert err <= bound, ("wlogsum", tag, float(got[0]), float(ref), err, bound)
    print("LogSum: largest error / bound: wlogsum %.3f, wave_logsum %.3f" % (worst["wlogsum"], worst["wave_logsum"]))
    return worst


def check_reductions(dump, info):
    worst = 0.0
    for k, cases in info["reduce"]:
        w = R.as_f64(dump[k])      # [case][4][lane]
        for ci, (tpb, name, v) in enumerate(cases):
            tag = "%s, %d threads" % (name, tpb)
            gs, gmax, gmin, gwm = w[ci]
            for arr, what in ((gs, "wsum"), (gmax, "wmax"), (gmin, "wmin")):
                assert all(R.same(float(x), float(arr[0])) for x in arr), ("lanes differ", what, tag)
            assert R.same(float(gs[0]), R.emu_wsum(v), zero_sign=False), ("wsum", tag, float(gs[0]), R.emu_wsum(v))
            assert R.same(float(gmax[0]), R.emu_wmax(v), zero_sign=False), ("wmax", tag, float(gmax[0]), R.emu_wmax(v))
            assert R.same(float(gmin[0]), R.emu_wmin(v), zero_sign=False), ("wmin", tag, float(gmin[0]), R.emu_wmin(v))
            for wv, want in enumerate(R.emu_wave_min(v)):
                assert all(R.same(float(x), want, zero_sign=False) for x in gwm[64 * wv:64 * wv + 64]), ("wave_min", tag, wv, float(gwm[64 * wv]), want)
            # the IEEE fmax / fmin behaviour, stated without the emulation: a NaN lane is ignored unless every lane is NaN; wsum propagates it
            fin = v[~np.isnan(v)]
            if fin.size:
                assert float(gmax[0]) == float(fin.max()) and float(gmin[0]) == float(fin.min()), ("nan lane not ignored", tag)
                for wv in range(tpb // 64):
                    fw = v[64 * wv:64 * wv + 64]
                    fw = fw[~np.isnan(fw)]
                    assert (math.isnan(gwm[64 * wv]) and fw.size == 0) or float(gwm[64 * wv]) == float(fw.min()), ("wave_min", tag, wv)
            else:
                assert math.isnan(gmax[0]) and math.isnan(gmin[0]) and np.isnan(gwm).all(), ("all nan", tag)
            if np.isnan(v).any() or (np.isinf(v).any() and (v == math.inf).any() and (v == -math.inf).any()):
                assert math.isnan(gs[0]), ("wsum must propagate", tag)
            elif np.isinf(v).any():
                assert float(gs[0]) == float(v[np.isinf(v)][0]), ("wsum", tag)
            else:
                bound = tpb * U * float(np.abs(v).sum())
                err = abs(float(gs[0]) - math.fsum(float(x) for x in v))
                worst = max(worst, err / bound if bound > 0 else 0.0)
                assert err <= bound, ("wsum against fsum", tag, err, bound)
    print("reductions: wsum largest error / (n u sum |v|) = %.4f" % worst)
    return worst


def check_index_and_bounds(dump, info):
    k, rows = info["pair"]
    w = R.as_f64(dump[k])
    for r, (m, q, a, b) in enumerate(rows.astype(int)):
        i, j = min(a, b), max(a, b)      # the table walks the lexicographic enumeration: row q of team size m is the pair (i, j)
        assert (int(w[r, 0]), int(w[r, 1])) == (i, j), ("pair_of", m, q, w[r, :2])
        if a < b:
            assert int(w[r, 2]) == q, ("pidx", m, a, b, w[r, 2])
        assert int(w[r, 3]) == q, ("pidx_any", m, a, b, w[r, 3])
    k, rows = info["bound"]
    w = R.as_f64(dump[k])
    for r in range(len(rows)):
        lo, bst, bvl, pc, ps = R.ref_bound_row(rows[r])
        got = [float(x) for x in w[r]]
        tag = tuple(rows[r][:7])
        assert R.same(got[0], lo) and R.same(got[5], lo), ("lbu", tag, got[0], got[5], lo)
        assert got[1] == bst, ("bst", tag, got[1], bst)
        assert R.same(got[2], bvl) and R.same(got[6], bvl), ("bvl", tag, got[2], got[6], bvl)
        assert R.same(got[3], pc) and R.same(got[7], pc), ("push_control", tag, got[3], got[7], pc)
        assert R.same(got[4], ps), ("push_state", tag, got[4], ps)
    return len(rows)


def check_rows(dump, info, exact):
    import mpmath
    k, rows = info["rows"]
    w = R.as_f64(dump[k])
    e0 = seed_error(dump, info)
    q = U if exact else e0 * e0 + 3 * U
    worst = {}
    for r in range(len(rows)):
        name = R.R_NAMES[int(rows[r, 0])]
        for o, (ref, bound) in enumerate(R.ref_row(rows[r], q)):
            got = float(w[r, o])
            err = float(abs(mpmath.mpf(got) - ref))
            key = name if len(R.ROW_C[name]) == 1 else "%s[%d]" % (name, o)
            worst[key] = max(worst.get(key, 0.0), err / bound)
            assert err <= bound, (key, tuple(rows[r]), got, float(ref), err, bound)
    print("row helpers (%s build): largest error / bound: " % ("exact" if exact else "product") + ", ".join("%s %.3f" % kv for kv in worst.items()))
    return worst


def host_controller(tmp_path, rows):
    """the same rows through csrc/nmpc_ipm.h as the host compiler builds it (the compiler and flags of tests/test_ipm_control_host.py)"""
    exe = tmp_path / "ipm_cases_host"
    r = subprocess.run([IH._compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + R.CSRC, os.path.join(R.PROBE_DIR, "ipm_cases_host.cpp"), "-o", str(exe), "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    (tmp_path / "rows.bin").write_bytes(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "rows.bin"), str(tmp_path / "host.bin")], check=True, timeout=60)
    return np.frombuffer((tmp_path / "host.bin").read_bytes(), dtype=np.float64).reshape(len(rows), R.IPM_OUT)


def check_controller(dump, info, host):
    k, rows, names = info["ipm"]
    dev = R.as_f64(dump[k])
    findings = []
    for r in range(len(rows)):
        name = names[r] if r < len(names) else "armijo (borderline)"
        if name == "barrier_update":      # pow comes from another library on the device
            mu0, tol = float(rows[r, 1]), float(rows[r, 2])
            assert R.barrier_reductions(mu0, float(dev[r, 0]), tol) == R.barrier_reductions(mu0, float(host[r, 0]), tol), (name, tuple(rows[r]), dev[r, 0], host[r, 0])
            assert R.ulps(float(dev[r, 0]), float(host[r, 0])) <= 4, (name, tuple(rows[r]), dev[r, 0], host[r, 0])
            continue
        if r >= len(names):
            # m_trial within an ulp of the threshold: the device may decide by a contracted right-hand side.  It must decide as ONE of the
            # evaluations a compiler may choose does, the same one on every row; which one is the finding.
            models = R.armijo_models(*[float(x) for x in rows[r, 1:6]])
            findings.append({n for n, v in models.items() if v == bool(dev[r, 0])})
            assert bool(host[r, 0]) == models["as written"], ("host armijo", tuple(rows[r]))
            continue
        assert all(R.same(float(a), float(b)) for a, b in zip(dev[r], host[r])), (name, tuple(rows[r]), dev[r], host[r])
    form = set.intersection(*findings) if findings else set()
    nborder = len(rows) - len(names)
    ndiff = sum(1 for r in range(len(names), len(rows)) if dev[r, 0] != host[r, 0])
    bu = [R.ulps(float(dev[r, 0]), float(host[r, 0])) for r in range(len(names)) if names[r] == "barrier_update"]
    print("controller: %d rows bit-equal to the host, barrier_update within %d ulp on %d rows; armijo at the threshold: %d of %d rows decided differently "
          "from the host; consistent with %s" % (len(names) - len(bu), max(bu), len(bu), ndiff, nborder, sorted(form)))
    assert form, "the device's armijo matches no single evaluation order on every borderline row"
    return form, ndiff, nborder


# ---------------------------------------------------------------- the tests
def test_reciprocals_and_division(probe):
    check_reciprocals(probe["fast"], probe["info"], exact=False)


def test_reciprocals_and_division_exact_build(probe):
    check_reciprocals(probe["exact"], probe["info"], exact=True)


def test_edge_table_and_divergence_from_ieee(probe):
    got = edge_divergence(probe["fast"], probe["info"])
    print("\n".join(edge_table(probe["fast"], probe["info"])))
    print("\n".join(got))
    assert got == documented("qdiv-vs-ieee"), "the (a, b) classes where qdiv leaves the IEEE division are not the ones docs/WAVE_PRIMITIVES.md lists"
    assert edge_table(probe["fast"], probe["info"]) == documented("edge-table")
    assert edge_divergence(probe["exact"], probe["info"]) == []


def test_logsum(probe):
    check_logsum(probe["fast"], probe["info"])


def test_reductions(probe):
    check_reductions(probe["fast"], probe["info"])


def test_index_and_bound_helpers(probe):
    check_index_and_bounds(probe["fast"], probe["info"])


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_row_helpers(probe, build):
    check_rows(probe[build], probe["info"], exact=build == "exact")


def test_controller_on_device(probe, tmp_path):
    host = host_controller(tmp_path, probe["info"]["ipm"][1])
    form, ndiff, nborder = check_controller(probe["fast"], probe["info"], host)
    assert documented("armijo-form") == sorted(form)
