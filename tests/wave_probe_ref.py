"""References for tests/probes/wave_probe.hip: the input tables it is given, exact models of what the probed primitives must return, and the
bounds the tests hold them to.  Plain Python: exact integer / fractions.Fraction arithmetic for a rounded fma, *, + and /, mpmath at 200
bits for log and sqrt, numpy for the order of the reductions.  Nothing here reads a kernel or a dump's expected value.

Bounds (u = 2^-53, e0 = the largest relative error of the v_rcp_f64 seed over the working domain D, measured from the dumped seeds):

  rcp1, rcp_nr   e0^2 + 2u.  With r0 = (1 + e) / d: t = fl(1 - d r0) = -e (1 + d1), r1 = fl(r0 + t r0) = (1 - e^2 - e d1 (1 + e)) (1 + d2) / d,
                 so the error is at most e0^2 + u (1 + e0 + ...) < e0^2 + u (1 + 2 e0): the 2u of the bound is not tight, it is kept.
  rcp2           2u: the second step squares e0^2 + 2u (< 2^-86) and adds its own rounding u (1 + ...).
  qdiv           e0^2 + 3u: one more rounding for the multiply.
  LogSum         |got - ref| <= 1.1 n u + 4u max(1, |ref|), n the number of terms: n - 1 rounded mantissa products (each moves the logarithm by
                 at most u (1 + u)), log of a mantissa in [0.5, 1) to one ulp (<= u), the rounded constant ln 2 (0.3u relative) and the final
                 fma (u) on a wave's sum, the cross-wave additions (W - 1 roundings of partial sums).  The last part is 4u |ref| only while the
                 wave sums share a sign (then every partial sum is at most |ref|: 1.3u + 2.25u for four equal waves); for waves of opposite
                 sign |ref| would have to read sum |ref_w|.  Every case of the table has same-sign wave sums; the test holds that first.
  wsum           n u sum |v| against math.fsum: n - 1 additions, each rounding at most u times a partial sum of absolute values.
  row helpers    c u S + nd q Q: c roundings of quantities bounded by S (the sum of the absolute summands), nd divisions of relative error q
                 (e0^2 + 3u, or u in the exact-division build) of a quotient bounded by Q.  ROW_C holds (c, nd) per helper and output.
"""
import math
import struct
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
DMAX = 1.7976931348623157e308
G_RCP, G_QDIV, G_LOGSUM, G_REDUCE, G_PAIR, G_BOUND, G_IPM, G_ROWS = 1, 2, 3, 4, 5, 6, 7, 8
WORDS = {G_RCP: 4, G_QDIV: 2, G_LOGSUM: 5, G_REDUCE: 4, G_PAIR: 4, G_BOUND: 8, G_IPM: 8, G_ROWS: 3}
PROBED = ["rcp1", "rcp2", "rcp_nr", "qdiv", "uniform_f64", "LogSum", "wsum", "wmax", "wmin", "wlogsum", "wave_min", "wave_logsum", "pidx", "pidx_any",
          "pair_of", "lbu", "bst", "bvl", "push_control", "push_state", "h_pair", "ds_pair", "r_obs", "h_obs", "ds_obs", "defect_xy", "defect_th",
          "ds_bound", "dz_of", "jd_pair", "jd_obs", "el_sigma", "el_step", "opt_error", "barrier_update", "frac_to_boundary", "shift_first",
          "shift_next", "shift_exhausted", "shift_accept", "penalty_update", "armijo", "watchdog_fires", "watchdog_count", "count_step",
          "cold_retry_left", "cold_retry_due", "cold_retry_begin", "stalled", "restarts_used_up", "barrier_restart_begin", "restart_mu"]


# ---------------------------------------------------------------- bits, classes, exact arithmetic
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def same(a, b, zero_sign=True):
    """equal as results: the same bits, or both NaN (payloads are not compared); zero_sign=False: +0 and -0 are the same"""
    if a != a or b != b:
        return a != a and b != b
    if a == 0.0 and b == 0.0 and not zero_sign:
        return True
    return bits(a) == bits(b)


def ordinal(x):
    b = bits(x)
    return b if b < (1 << 63) else (1 << 63) - b


def ulps(a, b):
    return abs(ordinal(a) - ordinal(b))


def fclass(x):
    if x != x:
        return "nan"
    if math.isinf(x):
        return "+inf" if x > 0 else "-inf"
    if x == 0.0:
        return "-0" if math.copysign(1.0, x) < 0 else "+0"
    return "finite"


def _dec(x):
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def _round(n, e):
    """n * 2^e, n an integer, correctly rounded to a double (to nearest even; overflow to an infinity)"""
    if n == 0:
        return 0.0
    try:
        return float(n << e) if e >= 0 else n / (1 << -e)
    except OverflowError:
        return math.inf if n > 0 else -math.inf


def fma(a, b, c):
    """IEEE-754 fma(a, b, c) = round(a b + c), one rounding, from exact integer arithmetic"""
    if a != a or b != b or c != c:
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return math.nan
        p = math.copysign(math.inf, math.copysign(1.0, a) * math.copysign(1.0, b))
        return math.nan if (math.isinf(c) and c != p) else p
    if math.isinf(c):
        return c
    sp = math.copysign(1.0, a) * math.copysign(1.0, b)
    if a == 0.0 or b == 0.0:
        if c == 0.0:
            return -0.0 if (sp < 0 and math.copysign(1.0, c) < 0) else 0.0
        return c
    (ma, ea), (mb, eb) = _dec(a), _dec(b)
    n, e = ma * mb, ea + eb
    if c != 0.0:
        mc, ec = _dec(c)
        lo = min(e, ec)
        n, e = (n << (e - lo)) + (mc << (ec - lo)), lo
        if n == 0:
            return 0.0
    r = _round(n, e)
    return math.copysign(0.0, sp if c == 0.0 else (1.0 if n > 0 else -1.0)) if r == 0.0 else r


def mul(a, b):
    return fma(a, b, -0.0)      # adding -0 changes no product, not a zero one's sign either


def ieee_div(a, b):
    """a / b as IEEE-754 defines it (Python raises where IEEE returns an infinity or a NaN)"""
    if a != a or b != b:
        return math.nan
    s = math.copysign(1.0, a) * math.copysign(1.0, b)
    if math.isinf(a):
        return math.nan if math.isinf(b) else math.copysign(math.inf, s)
    if math.isinf(b):
        return math.copysign(0.0, s)
    if b == 0.0:
        return math.nan if a == 0.0 else math.copysign(math.inf, s)
    if a == 0.0:
        return math.copysign(0.0, s)
    r = _round_fraction(Fraction(a) / Fraction(b))
    return math.copysign(0.0, s) if r == 0.0 else r


def _round_fraction(f):
    try:
        return f.numerator / f.denominator      # integer true division: correctly rounded, subnormals included
    except OverflowError:
        return math.inf if f > 0 else -math.inf


def newton(d, r):
    """one Newton step of the reciprocal as the headers write it: fma(fma(-d, r, 1), r, r)"""
    return fma(fma(-d, r, 1.0), r, r)


def rel_err_rcp(got, d):
    """|got - 1/d| / |1/d|, exact before the final conversion"""
    return float(abs(Fraction(got) * Fraction(d) - 1))


def rel_err_div(got, a, b):
    return float(abs(Fraction(got) * Fraction(b) / Fraction(a) - 1))


# ---------------------------------------------------------------- tables: reciprocals and divisions
def _pow2(e):
    return math.ldexp(1.0, e)


MIN_SUB, MAX_SUB, MIN_NORM = 5e-324, from_bits((1 << 52) - 1), _pow2(-1022)
EDGE_B = [("+0", 0.0), ("min_sub", MIN_SUB), ("max_sub", MAX_SUB), ("2^-1022", MIN_NORM), ("2^1022", _pow2(1022)), ("2^1023", _pow2(1023)),
          ("max", DMAX), ("inf", math.inf)]
EDGE_B = [(n if n == "+0" else "+" + n, v) for n, v in EDGE_B] + [("-" + n.lstrip("+"), -v) for n, v in EDGE_B] + [("nan", math.nan)]
EDGE_A = [("+0", 0.0), ("+1", 1.0), ("-1", -1.0), ("+tiny", 1e-300), ("-tiny", -1e-300), ("+huge", 1e300), ("-huge", -1e300), ("+inf", math.inf),
          ("-inf", -math.inf), ("nan", math.nan)]
SPECIAL_MANT = [1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, math.sqrt(2.0), math.pi / 2.0, math.e / 2.0, 1.1, 1.0 + 2.0 ** -26]


def rcp_table(seed=20241):
    """(values, n_D): the first n_D values are the working domain D (signs +-, exponents -300 .. 300); then every exponent -1022 .. 1023 at a
    handful of mantissas, the largest subnormals' neighbourhood, and the edge denominators"""
    rng = np.random.default_rng(seed)
    exps = list(range(-300, 301, 25))
    v = [s * math.ldexp(m, e) for e in exps for m in SPECIAL_MANT for s in (1.0, -1.0)]
    mant = 1.0 + rng.random(4096)
    for m in mant:
        for e in rng.integers(-300, 301, size=4):
            v.append(math.ldexp(m, int(e)) * (1.0 if rng.random() < 0.5 else -1.0))
    n_d = len(v)
    for e in range(-1022, 1024):
        for m in (1.0, 2.0 - 2.0 ** -52, math.sqrt(2.0), 1.0 + 2.0 ** -52, float(mant[e % 4096])):
            v.append(math.ldexp(m, e))
        v.append(-math.ldexp(float(mant[(e + 7) % 4096]), e))
    v += [x for _, x in EDGE_B]
    return np.array(v, dtype=np.float64), n_d


def qdiv_table(seed=20242):
    """(rows [n][2] of (a, b), n_D, edge index): the first n_D rows have b in D and a quotient in the normal range; then b at every exponent;
    then the edge table EDGE_A x EDGE_B, whose first row is edge index"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(12000):
        b = math.ldexp(1.0 + rng.random(), int(rng.integers(-300, 301))) * (1.0 if rng.random() < 0.5 else -1.0)
        a = math.ldexp(1.0 + rng.random(), int(rng.integers(-300, 301))) * (1.0 if rng.random() < 0.5 else -1.0)
        rows.append((a, b))
    for e in range(-300, 301, 25):
        for m in SPECIAL_MANT:
            b = math.ldexp(m, e)
            rows += [(1.0, b), (-b, b), (math.ldexp(SPECIAL_MANT[3], -e), -b), (3.0, b)]
    n_d = len(rows)
    for e in range(-1022, 1024):
        b = math.ldexp(1.0 + rng.random(), e)
        rows += [(1.0, b), (math.ldexp(1.0 + rng.random(), int(rng.integers(-300, 301))), -b)]
    edge = len(rows)
    rows += [(a, b) for _, a in EDGE_A for _, b in EDGE_B]
    return np.array(rows, dtype=np.float64), n_d, edge


def divergence(qdiv_of, tol):
    """the (a, b) classes of the edge table at which qdiv does not return what the IEEE division returns: another class, or a finite value
    further than tol (relative) from it.  qdiv_of(k): the probed result of edge row k.  Lines 'a b -> qdiv | ieee'."""
    out = []
    k = 0
    for na, a in EDGE_A:
        for nb, b in EDGE_B:
            got, want = qdiv_of(k), ieee_div(a, b)
            k += 1
            cg, cw = fclass(got), fclass(want)
            if cg != cw or (cg == "finite" and abs(got - want) > tol * abs(want)):
                out.append("%s / %s -> %s | %s" % (na, nb, cg, cw))
    return out


# ---------------------------------------------------------------- LogSum
def ref_logsum(terms):
    """sum of log(t) over positive finite doubles, as an mpmath number: exact products of the mantissas in chunks, one logarithm per chunk"""
    import mpmath
    with mpmath.workprec(200):
        acc, esum = mpmath.mpf(0), 0
        t = [float(x) for x in np.asarray(terms).ravel()]
        for i in range(0, len(t), 32):
            p = 1
            for x in t[i:i + 32]:
                m, e = _dec(x)
                p *= m
                esum += e
            acc += mpmath.log(mpmath.mpf(p))
        return acc + esum * mpmath.log(2)


def logsum_cases(seed=20243):
    """list of (tpb, name, terms [T][tpb], special): special None or the class of term planted ('zero', 'neg', 'nan', 'inf') with its lane"""
    rng = np.random.default_rng(seed)
    cases = []

    def logu(shape):
        return np.exp(rng.uniform(math.log(1e-12), math.log(1e4), size=shape))
    for tpb in (64, 128, 256):
        cases.append((tpb, "loguniform T=1", logu((1, tpb)), None))
        cases.append((tpb, "loguniform T=7", logu((7, tpb)), None))
        cases.append((tpb, "near 1e-300 T=64", 1e-300 * (1.0 + rng.random((64, tpb))), None))
        cases.append((tpb, "near 1e300 T=64", 1e300 * (1.0 + rng.random((64, tpb))), None))
        sub = (rng.integers(1, 1 << 52, size=(3, tpb), dtype=np.int64)).view(np.float64)
        cases.append((tpb, "subnormal T=3", sub, None))
        for lane in (0, 63, 64, 255):
            if lane >= tpb:
                continue
            for name, val in (("zero", 0.0), ("neg", -1.5), ("nan", math.nan), ("inf", math.inf)):
                t = logu((2, tpb))
                t[1, lane] = val
                cases.append((tpb, "%s in lane %d" % (name, lane), t, (name, lane)))
    cases.append((64, "near 1e-300 T=4096", 1e-300 * (1.0 + rng.random((4096, 64))), None))
    cases.append((64, "near 1e300 T=4096", 1e300 * (1.0 + rng.random((4096, 64))), None))
    cases.append((256, "near 1e-300 T=512", 1e-300 * (1.0 + rng.random((512, 256))), None))
    cases.append((256, "near 1e300 T=512", 1e300 * (1.0 + rng.random((512, 256))), None))
    return cases


def logsum_bound(n_terms, ref):
    return 1.1 * n_terms * U + 4.0 * U * max(1.0, abs(ref))


# ---------------------------------------------------------------- reductions
def butterfly(v, op):
    """what every lane of each 64-lane wave holds after v = op(v, v[lane ^ o]) for o = 32, 16, .., 1"""
    v = np.array(v, dtype=np.float64).reshape(-1, 64)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = op(v, v[:, idx ^ o])
    return v


def emu_wsum(v):
    w = butterfly(v, np.add)[:, 0]
    if len(w) == 1:
        return float(w[0])
    t = np.float64(0.0)
    with np.errstate(all="ignore"):
        for x in w:
            t = t + x
    return float(t)


def emu_wmax(v):
    w = butterfly(v, np.fmax)[:, 0]
    t = w[0]
    for x in w[1:]:
        t = np.fmax(t, x)
    return float(t)


def emu_wmin(v):
    return -emu_wmax(-np.asarray(v, dtype=np.float64))


def emu_wave_min(v):
    return [float(x) for x in butterfly(v, np.fmin)[:, 0]]      # one value per wave


def reduce_cases(seed=20244):
    """list of (tpb, name, values [tpb])"""
    rng = np.random.default_rng(seed)
    cases = []
    for tpb in (64, 128, 256):
        for k in range(3):
            cases.append((tpb, "mixed magnitudes %d" % k, rng.standard_normal(tpb) * np.exp2(rng.integers(-30, 31, size=tpb))))
        c = rng.standard_normal(tpb)
        c[1::2] = -c[0::2] * (1.0 + 1e-9 * rng.standard_normal(tpb // 2))
        cases.append((tpb, "cancelling", c))
        cases.append((tpb, "positive", rng.random(tpb) + 0.5))
        for lane in sorted({0, 63, tpb - 1, tpb // 2}):
            x = rng.standard_normal(tpb)
            x[lane] = math.nan
            cases.append((tpb, "nan in lane %d" % lane, x))
        if tpb > 64:
            x = rng.standard_normal(tpb)
            x[64:128] = math.nan
            cases.append((tpb, "wave 1 all nan", x))
        cases.append((tpb, "all nan", np.full(tpb, math.nan)))
        x = rng.standard_normal(tpb); x[tpb - 3] = math.inf
        cases.append((tpb, "+inf lane", x))
        x = rng.standard_normal(tpb); x[5] = -math.inf
        cases.append((tpb, "-inf lane", x))
        x = rng.standard_normal(tpb); x[5] = -math.inf; x[tpb - 3] = math.inf
        cases.append((tpb, "+inf and -inf", x))
        cases.append((tpb, "mixed zeros", np.where(rng.random(tpb) < 0.5, 0.0, -0.0)))
        cases.append((tpb, "all -0", np.full(tpb, -0.0)))
    return cases


# ---------------------------------------------------------------- index and bound helpers
def pair_rows():
    """rows (M, q, a, b) for M = 2 .. 10: every pair in lexicographic order, as (i, j) and as (j, i)"""
    rows = []
    for m in range(2, 11):
        q = 0
        for i in range(m):
            for j in range(i + 1, m):
                rows += [(m, q, i, j), (m, q, j, i)]
                q += 1
        assert q == m * (m - 1) // 2
    return np.array(rows, dtype=np.float64)


BOUND_PUSH = 1e-2      # IPOPT bound_push = bound_frac
BOUND_SETS = [(0.26, 1.82, 20.0, math.pi), (2.5, 0.5, 0.3, 7.0)]      # (vmax, wmax, xymax, thmax): |bound| above and below 1, 2 b below max(1, b)


def bound_rows():
    rows = []
    for vmax, wmax, xymax, thmax in BOUND_SETS:
        vals = {0.0, 0.05, -0.05, 1e3, -1e3}
        for b in (vmax, wmax, xymax, thmax):
            for x in (b, math.nextafter(b, 0.0), math.nextafter(b, math.inf), 0.99 * b, b * (1.0 - BOUND_PUSH), 0.995 * b, 2.0 * b):
                vals |= {x, -x}
        for thb in (0, 1):
            for c in range(12):
                rows += [(thb, c, v, vmax, wmax, xymax, thmax, 0.0) for v in sorted(vals)]
    return np.array(rows, dtype=np.float64)


def ipopt_push(v, lo, hi):
    """IPOPT's push of a start value into the interior of [lo, hi]: both perturbations min(k1 max(1, |bound|), k2 (hi - lo)), k1 = k2 = bound_push"""
    f = np.float64
    pl = min(f(BOUND_PUSH) * max(f(1.0), abs(f(lo))), f(BOUND_PUSH) * (f(hi) - f(lo)))
    pu = min(f(BOUND_PUSH) * max(f(1.0), abs(f(hi))), f(BOUND_PUSH) * (f(hi) - f(lo)))
    return float(min(max(f(v), f(lo) + pl), f(hi) - pu))


def ref_bound_row(row):
    """(lbu, bst, bvl, push_control, push_state) of one row of bound_rows()"""
    thb, c, v, vmax, wmax, xymax, thmax = int(row[0]), int(row[1]), row[2], row[3], row[4], row[5], row[6]
    lo = -wmax if c & 1 else -vmax
    bst = c if thb else 3 * (c >> 1) + (c & 1)
    bvl = thmax if (thb and c % 3 == 2) else xymax
    pc = ipopt_push(v, lo, -lo)
    d = c % 3
    ps = v
    if d < 2 or thb:
        b = thmax if d == 2 else xymax
        ps = ipopt_push(v, -b, b)
    return lo, float(bst), bvl, pc, ps


# ---------------------------------------------------------------- row helpers
R_NAMES = ["h_pair", "ds_pair", "r_obs", "h_obs", "ds_obs", "defect_xy", "defect_th", "ds_bound", "dz_of", "jd_pair", "jd_obs", "el_sigma", "el_step"]
# (c, nd) per helper and output: c roundings of quantities bounded by S, nd divisions (module docstring).  Counted from the header:
#   h_pair     ey*ey, the fma, the subtraction
#   ds_pair    h_pair's three, the product, the fma, h - s, the sum
#   r_obs      the inner two halve under the root (relative), plus the root's own
#   h_obs      three subtractions
#   ds_obs     product and fma of the numerator, h - s, the sum; one division
#   defect_*   the fma, the subtraction;  ds_bound  h - s, the sum;  jd_pair  product, fma;  jd_obs  product, fma, one division
#   dz_of      two fmas of the numerator; one division
#   el_sigma   sg = 1 / D, D = s/z + t/(rho - z): rho - z, the sum (2), divisions: two of D count once each (positive terms), then 1 / D (2)
#              v = z - q sg: q's three (rho - z, two sums) on S_q, sg's two, the product and the subtraction (7); divisions: q's one, sg's two (3)
#   el_step    dz = -(jd + q) / D: q's three, the sum, D's two (6); divisions q, D, the quotient (3)
#              ds = (mu - s z - s dz) / z: two products, two subtractions (4), one division, plus (s / z) times dz's bound
#              dt = (mu - t rz + t dz) / rz: the same with rho - z in the product and the quotient (6), one division, plus (t / rz) times dz's bound
ROW_C = {"h_pair": [(3, 0)], "ds_pair": [(7, 0)], "r_obs": [(2, 0)], "h_obs": [(3, 0)], "ds_obs": [(4, 1)], "defect_xy": [(2, 0)], "defect_th": [(2, 0)],
         "ds_bound": [(2, 0)], "dz_of": [(2, 1)], "jd_pair": [(2, 0)], "jd_obs": [(2, 1)], "el_sigma": [(2, 2), (7, 3)], "el_step": [(4, 1), (6, 3), (6, 1)]}      # el_sigma: (sg, v); el_step: (ds, dz, dt)
RHO = 100.0


def rows_table(seed=20245, n=200):
    """rows (helper, seven arguments) in the solver's range"""
    rng = np.random.default_rng(seed)

    def lu(lo, hi):
        return float(np.exp(rng.uniform(math.log(lo), math.log(hi))))

    def sg(x):
        return x if rng.random() < 0.5 else -x
    rows = []
    for k in range(n):
        ex, ey, ddx, ddy = sg(lu(1e-3, 10.0)), sg(lu(1e-3, 10.0)), sg(lu(1e-9, 1.0)), sg(lu(1e-9, 1.0))
        dmin2 = 0.09 if k % 2 else lu(1e-2, 1.0)
        h = ex * ex + ey * ey - dmin2
        near = k % 3 == 0      # a slack that nearly cancels the row's value
        sv = abs(h) * (1.0 + sg(lu(1e-12, 1e-6))) if near else lu(1e-12, 1e6)
        zv, mu = lu(1e-12, 1e6), lu(1e-9, 1.0)
        rr = math.hypot(ex, ey)
        robdim, orad, margin = lu(0.05, 0.5), lu(0.05, 2.0), lu(1e-3, 0.2)
        hv = rr - robdim - orad - margin
        so = abs(hv) * (1.0 + sg(lu(1e-12, 1e-6))) if near else lu(1e-12, 1e6)
        rows.append((0, ex, ey, dmin2, 0, 0, 0, 0))
        rows.append((1, ex, ey, ddx, ddy, dmin2, sv, 0))
        rows.append((2, ex, ey, 0, 0, 0, 0, 0))
        rows.append((3, rr, robdim, orad, margin, 0, 0, 0))
        rows.append((4, ex, ey, rr, ddx, ddy, hv, so))
        xn, x, tu, cs = sg(lu(1e-3, 20.0)), sg(lu(1e-3, 20.0)), sg(lu(1e-4, 0.1)), sg(rng.random())
        if near:
            xn = x + tu * cs * (1.0 + 1e-9)
        rows.append((5, xn, x, tu, cs, 0, 0, 0))
        rows.append((6, xn, x, 0.1, sg(lu(1e-3, 2.0)), 0, 0, 0))
        rows.append((7, sg(lu(1e-9, 1.0)), h, sv, 0, 0, 0, 0))
        rows.append((8, mu, lu(1e-12, 1e6), zv, sg(lu(1e-9, 10.0)), 0, 0, 0))
        rows.append((9, ex, ey, ddx, ddy, 0, 0, 0))
        rows.append((10, ex, ey, rr, ddx, ddy, 0, 0))
        zel = RHO - lu(1e-12, 50.0) if k % 4 == 0 else lu(1e-12, 99.0)      # the dual of an elastic row lies in (0, rho), near either end
        tv, sel = lu(1e-12, 1e6), lu(1e-12, 1e6)
        rows.append((11, mu, RHO, sel, zel, tv, h, 0))
        rows.append((12, mu, RHO, sel, zel, tv, h, sg(lu(1e-9, 1.0))))
    return np.array(rows, dtype=np.float64)


def ref_row(row, q):
    """[(reference, bound)] per output of one row of rows_table(); q: the relative error allowed to one division"""
    import mpmath
    with mpmath.workprec(200):
        mp = mpmath.mpf
        a = [mp(float(x)) for x in row[1:]]
        name = R_NAMES[int(row[0])]
        cs = ROW_C[name]

        def B(k, S, Q=0):
            c, nd = cs[k]
            return float((c * U * S + nd * q * Q) * (1 + mp(2) ** -20))
        if name == "h_pair":
            ex, ey, d2 = a[:3]
            return [(ex * ex + ey * ey - d2, B(0, ex * ex + ey * ey + d2))]
        if name == "ds_pair":
            ex, ey, dx, dy, d2, sv = a[:6]
            return [(2 * ex * dx + 2 * ey * dy + (ex * ex + ey * ey - d2 - sv), B(0, abs(2 * ex * dx) + abs(2 * ey * dy) + ex * ex + ey * ey + d2 + abs(sv)))]
        if name == "r_obs":
            r = mpmath.sqrt(a[0] * a[0] + a[1] * a[1])
            return [(r, B(0, r))]
        if name == "h_obs":
            return [(a[0] - a[1] - a[2] - a[3], B(0, abs(a[0]) + abs(a[1]) + abs(a[2]) + abs(a[3])))]
        if name in ("ds_obs", "jd_obs"):
            ex, ey, rr, d0, d1 = a[:5]
            Q = (abs(ex * d0) + abs(ey * d1)) / abs(rr)
            jd = (ex * d0 + ey * d1) / rr
            if name == "jd_obs":
                return [(jd, B(0, Q, Q))]
            return [(jd + (a[5] - a[6]), B(0, Q + abs(a[5]) + abs(a[6]), Q))]
        if name in ("defect_xy", "defect_th"):
            return [(a[0] - (a[2] * a[3] + a[1]), B(0, abs(a[0]) + abs(a[2] * a[3]) + abs(a[1])))]
        if name == "ds_bound":
            return [(a[0] + (a[1] - a[2]), B(0, abs(a[0]) + abs(a[1]) + abs(a[2])))]
        if name == "dz_of":
            mu, sv, zv, ds = a[:4]
            Q = (abs(zv * ds) + abs(sv * zv) + abs(mu)) / abs(sv)
            return [((mu - sv * zv - zv * ds) / sv, B(0, Q, Q))]
        if name == "jd_pair":
            return [(2 * a[0] * a[2] + 2 * a[1] * a[3], B(0, abs(2 * a[0] * a[2]) + abs(2 * a[1] * a[3])))]
        mu, rho, sv, zv, tv, hv = a[:6]
        rz = rho - zv
        D = sv / zv + tv / rz
        qq = hv - mu / zv + mu / rz
        Sq = abs(hv) + mu / zv + mu / rz
        if name == "el_sigma":
            sgm = 1 / D
            return [(sgm, B(0, sgm, sgm)), (zv - qq * sgm, B(1, abs(zv) + Sq * sgm, Sq * sgm))]
        jd = a[6]
        Sn = (abs(jd) + Sq) / D
        dz = -(jd + qq) / D
        bdz = B(1, Sn, Sn)
        S2 = (mu + sv * zv + sv * abs(dz)) / zv
        S3 = (mu + tv * rz + tv * abs(dz)) / rz
        return [((mu - sv * zv - sv * dz) / zv, B(0, S2, S2) + float(sv / zv) * bdz * (1 + 2.0 ** -20)), (dz, bdz),
                ((mu - tv * rz + tv * dz) / rz, B(2, S3, S3) + float(tv / rz) * bdz * (1 + 2.0 ** -20))]


# ---------------------------------------------------------------- the controller: the inputs of tests/test_ipm_control_host.py as table rows
OPT_ERROR, BARRIER_UPDATE, FRAC_TO_BOUNDARY, SHIFT, SHIFT_ACCEPT, PENALTY_UPDATE, MERIT_REF, ARMIJO, WATCHDOG, LADDER, RESTART_MU = range(11)
IPM_IN, IPM_OUT = 12, 8
WATCHDOG_TRIGGER, WATCHDOG_MIN_AP, COLD_RETRY_ITERS, COLD_RETRIES, SHIFT_ESCALATION = 10, 0.5, 500, 2, 8.0      # include/nmpc_constants.h


def ipm_rows():
    """(rows [n][12], names [n]): one rule call per row (tests/probes/ipm_cases.h).  The rules with state (shift schedule, merit reference,
    ladder) are walked with the state a plain restatement of the rule gives, so every row stands alone."""
    rows, names = [], []

    def add(name, fn, *args):
        rows.append([float(fn)] + [float(x) for x in args] + [0.0] * (IPM_IN - 1 - len(args)))
        names.append(name)
    for a in ((3.0, 0.25, 0.5, 1000.0, 500.0, 2.0, 10.0, 6.0), (3.0, 0.25, 0.5, 4000.0, 2000.0, 8.0, 10.0, 6.0), (3.0, 0.25, 0.5, 4000.0, 2000.0, 8.0, 4.0, 1.0)):
        add("opt_error", OPT_ERROR, *a)
    for a in ((0.5, 1e-8, 0, 0, 0, 0, 0, 1), (0.5, 1e-8, 0, 0.5, 0, 0, 0, 1), (0.5, 1e-8, 0, 0.15, 0, 0, 0, 1), (0.5, 1e-8, 0, 6.0, 0, 0, 0, 1),
              (0.5, 1e-8, 6.0, 0, 0, 0, 0, 1), (0.5, 1e-8, 0, 0, 6.0, 0, 0, 1), (0.5, 1e-8, 0, 0, 0, 6.5, 0.5, 1), (0.5, 1e-8, 0, 0, 0, 6.5, 0.5, 2),
              (1e-9, 1e-8, 0, 0, 0, 0, 0, 1)):
        add("barrier_update", BARRIER_UPDATE, *a)
    for mu in (0.5, 1e-3):
        add("frac_to_boundary", FRAC_TO_BOUNDARY, mu)
    for dl in (0.0, 3e-3):      # the schedule from no shift until it is exhausted
        d = 0.0
        while True:
            add("shift", SHIFT, 0, d, dl)
            if d > 1e20:
                break
            d = ((1e-4 if dl == 0.0 else max(1e-20, dl / 3.0)) if d == 0.0 else d * (100.0 if dl == 0.0 else SHIFT_ESCALATION))
    for need, dl in ((1, 3e-3), (1, 1e-21), (0, 3e-3)):
        add("shift", SHIFT, need, 0.0, dl)
    for delta, ntry, dl in ((0.0, 0, 7e-2), (1e-4, 1, 0.0), (1e-7, 0, 7e-2), (1e-7, 1, 7e-2), (2e-6, 0, 7e-2)):
        add("shift_accept", SHIFT_ACCEPT, delta, ntry, dl, 1)
    for a in ((8.0, -1.0, 2.0, 100.0), (1.5, -1.0, 2.0, 100.0), (1.0, 9.0, 2.0, 100.0), (1.0, 900.0, 2.0, 18.0), (20.0, 9.0, 2.0, 100.0)):
        add("penalty_update", PENALTY_UPDATE, *a)
    st = [0.0, 0.0, 0.0, -1.0, -1.0, 0]      # h0, h1, h2, mu, nu, count
    calls = [(0.1, 1.0, m0, 0) for m0 in (5.0, 3.0, 4.0, 1.0, 0.5, 0.25)] + [(0.02, 1.0, 0.1, 0), (0.02, 1.0, 0.05, 0), (0.02, 2.0, 0.01, 0), (0.02, 2.0, 0.005, 0),
                                                                           (0.02, 2.0, 0.001, 1), (0.02, 2.0, 0.0005, 0)]
    for mu_, nu_, m0, reset in calls:
        add("merit_ref", MERIT_REF, *st, mu_, nu_, m0, reset)
        if reset or st[3] != mu_ or st[4] != nu_:
            st[5] = 0
        st[3], st[4] = mu_, nu_
        st[0], st[1], st[2], st[5] = m0, st[0], st[1], min(3, st[5] + 1)
    for a in ((1.0, 1.0, 0.5, -2.0, 0.0), (1.0 - 1e-4, 1.0, 0.5, -2.0, 0.0), (1.0 + 5e-14, 1.0, 0.5, 0.0, 1.0), (1.0 + 2e-13, 1.0, 0.5, 0.0, -1.0)):
        add("armijo", ARMIJO, *a)
    for n_short, took, alpha, a_p in ((WATCHDOG_TRIGGER - 1, 0, 0.5, 1.0), (WATCHDOG_TRIGGER, 0, 0.5, 1.0), (WATCHDOG_TRIGGER, 0, 0.25, 0.49),
                                      (WATCHDOG_TRIGGER, 0, 0.25, WATCHDOG_MIN_AP), (3, 0, 0.5, 1.0), (3, 0, 1.0, 1.0), (3, 1, 0.5, 1.0)):
        add("watchdog", WATCHDOG, n_short, took, alpha, a_p)
    lad = [0, 0, 0, 0]      # n_tiny, n_restart, n_cold, it_base
    it = 0
    for alpha in (1e-11, 1e-11, 1.0):
        add("ladder", LADDER, *lad, alpha, it, 0)
        lad[0] = lad[0] + 1 if alpha < 1e-10 else 0
    while True:      # tiny steps until the solve gives up
        it += 1
        tiny = lad[0] + 1
        act = 0
        if tiny >= 5:
            act = 1 if lad[1] < 3 else (2 if lad[2] < COLD_RETRIES else 3)
        add("ladder", LADDER, *lad, 1e-11, it, act if act < 3 else 0)
        lad[0] = tiny
        if act == 1:
            lad[1] += 1; lad[0] = 0
        if act == 2:
            lad = [0, 0, lad[2] + 1, it]
        if act == 3:
            break
    for lad, it in (([0, 0, 0, 0], COLD_RETRY_ITERS - 1), ([0, 0, 0, 0], COLD_RETRY_ITERS), ([0, 0, 1, COLD_RETRY_ITERS], 2 * COLD_RETRY_ITERS - 1),
                    ([0, 0, 1, COLD_RETRY_ITERS], 2 * COLD_RETRY_ITERS), ([0, 0, 2, 2 * COLD_RETRY_ITERS], 10 * COLD_RETRY_ITERS)):
        add("ladder", LADDER, *lad, 1.0, it, 2 if lad[2] < COLD_RETRIES and it % COLD_RETRY_ITERS == 0 else 0)
    for a in ((1e-6, 0.5), (2.0, 0.5)):
        add("restart_mu", RESTART_MU, *a)
    return np.array(rows, dtype=np.float64), names


def barrier_reductions(mu0, mu, tol):
    """how many times the rule mu <- max(tol / 10, min(0.2 mu, mu^1.5)) was applied to get from mu0 to (about) mu"""
    n, m = 0, mu0
    while m > mu * (1.0 + 1e-9):
        m = max(tol / 10.0, min(0.2 * m, m ** 1.5))
        n += 1
        if n > 200:
            break
    return n


def armijo_border_rows():
    """armijo rows at which m_trial sits within an ulp or two of the threshold mref + 1e-4 alpha Dm + 1e-13 |phi0|: a contracted and an
    uncontracted evaluation of the right-hand side can decide them differently.  Returns rows [n][12]."""
    rows = []
    rng = np.random.default_rng(20246)
    for _ in range(64):
        # all three terms of one magnitude: the rounding of each product then reaches the last bit of the sum
        mref, alpha, Dm, phi0 = float(rng.random() + 0.5), float(rng.random()), -float(rng.random() * 3e4), float(rng.standard_normal() * 1e13)
        thr = float(np.float64(mref) + np.float64(1e-4) * np.float64(alpha) * np.float64(Dm) + np.float64(1e-13) * abs(np.float64(phi0)))
        for k in (-1, 0, 1):
            m = thr
            for _ in range(abs(k)):
                m = math.nextafter(m, math.inf if k > 0 else -math.inf)
            rows.append([float(ARMIJO), m, mref, alpha, Dm, phi0] + [0.0] * (IPM_IN - 6))
    return np.array(rows, dtype=np.float64)


def armijo_models(m_trial, mref, alpha, Dm, phi0):
    """the decision under the evaluations of mref + 1e-4 alpha Dm + 1e-13 |phi0| a compiler may choose: (as written, inner fma, both fmas)"""
    f = np.float64
    t = float(f(1e-4) * f(alpha))
    plain = float(f(mref) + f(t) * f(Dm) + f(1e-13) * abs(f(phi0)))
    inner = fma(t, Dm, mref)
    one = float(f(inner) + f(1e-13) * abs(f(phi0)))
    both = fma(1e-13, abs(phi0), inner)
    outer_only = fma(1e-13, abs(phi0), float(f(mref) + f(t) * f(Dm)))
    return {"as written": m_trial <= plain, "fma(t, Dm, mref) + p": m_trial <= one, "fma(c, |phi0|, fma(t, Dm, mref))": m_trial <= both,
            "fma(c, |phi0|, mref + t Dm)": m_trial <= outer_only}


# ---------------------------------------------------------------- the files
def write_tables(path, sections):
    """sections: list of (id, array of shape (a, b) or (a, b, c))"""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(sections)))
        for gid, arr in sections:
            arr = np.ascontiguousarray(arr, dtype=np.float64)
            a, b, c = arr.shape if arr.ndim == 3 else (arr.shape[0], arr.shape[1], 1)
            f.write(struct.pack("<4q", gid, a, b, c))
            f.write(arr.tobytes())


def read_dump(path, sections):
    """list of uint64 arrays, one per section, shaped (a, words) or (a, words, lanes); checks the dump's headers against the tables'"""
    out = []
    with open(path, "rb") as f:
        (n,) = struct.unpack("<q", f.read(8))
        assert n == len(sections), (n, len(sections))
        for gid, arr in sections:
            h = struct.unpack("<4q", f.read(32))
            lanes = arr.shape[2] if gid in (G_LOGSUM, G_REDUCE) else 1
            assert h == (gid, arr.shape[0], WORDS[gid], lanes), (h, gid, arr.shape)
            cnt = h[1] * h[2] * h[3]
            d = np.frombuffer(f.read(8 * cnt), dtype=np.uint64)
            assert d.size == cnt
            out.append(d.reshape((h[1], h[2], h[3]) if lanes > 1 else (h[1], h[2])))
        assert f.read(1) == b""
    return out


def as_f64(w):
    return np.asarray(w, dtype=np.uint64).view(np.float64)


def all_sections():
    """(sections for write_tables, info): every group's tables in one file.  info holds what the assertions need besides the arrays."""
    info = {}
    sec = []
    rcp, n_d = rcp_table()
    info["rcp"] = (len(sec), rcp, n_d); sec.append((G_RCP, rcp.reshape(-1, 1)))
    qd, qn_d, edge = qdiv_table()
    info["qdiv"] = (len(sec), qd, qn_d, edge); sec.append((G_QDIV, qd))
    groups = {}
    for case in logsum_cases():
        groups.setdefault((case[0], case[2].shape[0]), []).append(case)
    info["logsum"] = []
    for (tpb, T), cs in sorted(groups.items()):
        info["logsum"].append((len(sec), cs)); sec.append((G_LOGSUM, np.stack([c[2] for c in cs])))
    info["reduce"] = []
    for tpb in (64, 128, 256):
        cs = [c for c in reduce_cases() if c[0] == tpb]
        info["reduce"].append((len(sec), cs)); sec.append((G_REDUCE, np.stack([c[2] for c in cs]).reshape(len(cs), 1, tpb)))
    pr = pair_rows()
    info["pair"] = (len(sec), pr); sec.append((G_PAIR, pr))
    br = bound_rows()
    info["bound"] = (len(sec), br); sec.append((G_BOUND, br))
    ir, names = ipm_rows()
    ir = np.concatenate([ir, armijo_border_rows()])
    info["ipm"] = (len(sec), ir, names); sec.append((G_IPM, ir))
    rr = rows_table()
    info["rows"] = (len(sec), rr); sec.append((G_ROWS, rr))
    return sec, info


# ---------------------------------------------------------------- building the probe
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nonlinear-mpc-for-collision-free-and-deadlock-free-navigation-of-multiple-nonholonomic-mobile-robots_amd")
CSRC = os.path.join(PKG, "csrc")
PROBE_DIR = os.path.join(ROOT, "tests", "probes")
PROBE_SRC = os.path.join(PROBE_DIR, "wave_probe.hip")
EXACT_DEFS = ["-DNMPC_FAST_DIV=0", "-DNMPC_RCP_STEPS=2"]      # the exact-arithmetic build: IEEE divisions, two Newton steps on a pivot


def build_module():
    """the package's build.py, loaded from its file (the package itself loads the library on import)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("nmpc_build_for_probe", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hipcc():
    return next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)


def probe_command(exe, extra=()):
    return [hipcc()] + build_module().codegen_flags() + list(extra) + ["-I" + CSRC, "-I" + PROBE_DIR, PROBE_SRC, "-o", str(exe)]


def compile_probe(exe, extra=()):
    r = subprocess.run(probe_command(exe, extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)
