"""CPU restatement of pair_side_kernel's summation and its certified slack (epi_refine.hip).

The kernel regroups the O(n) terms of e'Pe and eff so that what depends on the first SNP alone is
formed once per individual and shared by the pairs of a group:
    g1 = a (al z - u), g3 = diag(P) a^2, g5 = (a - al) Py, g6 = |a| (|u| + |al| |z|), g5m = |g5| + 2^-23 |al Py|
    sum w (al be z - be u - al v) = be sum b g1 - al sum (b a) v,   eff = sum b g5 - be sum g5
in fp32 (U in fp16), lane l of the wave adding individuals 512 t + 8 l + h in the order (t, h), even and odd h
to separate partial sums (two individuals per packed instruction), the two joined and the 64 lane partials
added in an fp32 butterfly, the combinations in fp64.  This file evaluates exactly that in numpy (an FMA
as the fp32 rounding of the fp64 product-sum: the product of two fp32 numbers is exact in fp64, so it differs from a hardware FMA by
a second rounding of 2^-29 relative at most) and checks |value - exact| <= slack against a long-double
evaluation from the unrounded inputs.
"""
import numpy as np
import pytest

F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _lanes(v, dtype):
    """individual 512 t + 8 l + h -> [t][l][h], zero-padded to whole iterations of the wave"""
    n = v.size
    out = np.zeros(-(-n // 512) * 512, dtype)
    out[:n] = v
    return out.reshape(-1, 64, 8)


def pair_side(a, b, ua, ub, z, dg, py, al, be):
    """(side, side_slack, eff, eff_slack, sum w^2) of one pair as the kernel forms them, without the host
    terms t3 .. t7 (fp64 products of per-SNP constants: their part of the slack is 1e-10 relative)."""
    n_pad = a.size
    with np.errstate(over="ignore", invalid="ignore"):
        u16, v16 = ua.astype(np.float16), ub.astype(np.float16)
        A, B = _lanes(a, F), _lanes(b, F)
        U, V = _lanes(u16.astype(F), F), _lanes(v16.astype(F), F)
        Z, D, Y = _lanes(z.astype(F), F), _lanes(dg.astype(F), F), _lanes(py.astype(F), F)
        alf = np.full(64, F(al))
        acc = {k: np.zeros((2, 64), F) for k in ("sA", "sAa", "sB", "sBa", "s2", "s2a", "s3", "s3a", "sw", "ef", "efa", "g5s", "g5ms")}
        for t in range(A.shape[0]):
            for h in range(8):
                av, bv, uu, vv, zz, d, y = (x[t, :, h] for x in (A, B, U, V, Z, D, Y))
                aav = np.abs(av)
                g1 = (av * _fma(alf, zz, -uu)).astype(F)
                g6 = (aav * _fma(np.abs(alf), np.abs(zz), np.abs(uu))).astype(F)
                g3 = (d * (av * av).astype(F)).astype(F)
                g5 = ((av - alf).astype(F) * y).astype(F)
                g5m = _fma(np.full(64, F(2.0 ** -23)), np.abs((alf * y).astype(F)), np.abs(g5))
                c = h & 1                                      # even and odd individuals: separate partial sums
                acc["g5s"][c] = (acc["g5s"][c] + g5).astype(F)
                acc["g5ms"][c] = (acc["g5ms"][c] + g5m).astype(F)
                ba, b2 = (bv * av).astype(F), (bv * bv).astype(F)
                acc["sA"][c] = _fma(bv, g1, acc["sA"][c])
                acc["sAa"][c] = _fma(np.abs(bv), g6, acc["sAa"][c])
                acc["sB"][c] = _fma(ba, vv, acc["sB"][c])
                acc["sBa"][c] = _fma(np.abs(ba), np.abs(vv), acc["sBa"][c])
                acc["s2"][c] = _fma(av, vv, acc["s2"][c])
                acc["s2a"][c] = _fma(aav, np.abs(vv), acc["s2a"][c])
                acc["s3"][c] = _fma(b2, g3, acc["s3"][c])
                acc["s3a"][c] = _fma(b2, np.abs(g3), acc["s3a"][c])
                acc["sw"][c] = _fma(ba, ba, acc["sw"][c])
                acc["ef"][c] = _fma(bv, g5, acc["ef"][c])
                acc["efa"][c] = _fma(np.abs(bv), g5m, acc["efa"][c])

        def wsum(v):  # the wave's butterfly over lane ^ 1, 2, ..., 32, in fp32
            r = (v[0] + v[1]).astype(F)
            for off in (1, 2, 4, 8, 16, 32):
                r = (r + r[np.arange(64) ^ off]).astype(F)
            return float(r[0])

        r = {k: wsum(v) for k, v in acc.items()}
        ab = al * be
        s1 = be * r["sA"] - al * r["sB"]
        s1a = abs(be) * r["sAa"] + abs(al) * r["sBa"]
        side = r["s3"] + 2.0 * s1 + 2.0 * ab * r["s2"]
        fsl = 2.0 * (n_pad // 64 + 8) * 2.0 ** -24
        su = 2.0 * s1a + 2.0 * abs(ab) * r["s2a"]
        slack = (fsl * (su + r["s3a"]) + 2.0 ** -10 * su + 2.0 ** -23 * (abs(al) + abs(be)) * 4.0 * n_pad
                 + 1e-10 * (r["s3a"] + su))
        eff = r["ef"] - be * r["g5s"]
        eff_slack = (fsl + 1e-10) * (r["efa"] + abs(be) * r["g5ms"])
    return side, slack, eff, eff_slack, r["sw"]


def exact(a, b, ua, ub, z, dg, py, al, be):
    L = np.longdouble
    a, b, ua, ub, z, dg, py = (x.astype(L) for x in (a, b, ua, ub, z, dg, py))
    al, be = L(al), L(be)
    w = a * b
    side = (dg * w * w).sum() + 2 * (w * (al * be * z - be * ua - al * ub)).sum() + 2 * al * be * (a * ub).sum()
    eff = ((a - al) * (b - be) * py).sum()
    return float(side), float(eff), float((w * w).sum())


def _inputs(rng, n_pad, n, scale_u):
    a = np.zeros(n_pad)
    b = np.zeros(n_pad)
    a[:n] = rng.integers(0, 3, n)
    b[:n] = rng.integers(0, 3, n)
    v = [np.zeros(n_pad) for _ in range(5)]
    for x in v:
        x[:n] = rng.standard_normal(n)
    ua, ub, z, dg, py = v
    ua *= scale_u(rng, n_pad)
    ub *= scale_u(rng, n_pad)
    dg = np.abs(dg) + 0.5
    dg[n:] = 0.0
    return a, b, ua, ub, z, dg, py


def _check(args):
    side, slack, eff, eff_slack, sw = pair_side(*args)
    x_side, x_eff, x_sw = exact(*args)
    assert np.isfinite(slack) and np.isfinite(eff_slack)
    assert abs(side - x_side) <= slack, (side, x_side, slack)
    assert abs(eff - x_eff) <= eff_slack, (eff, x_eff, eff_slack)
    assert sw == x_sw
    return abs(side - x_side) / slack, abs(eff - x_eff) / eff_slack


@pytest.mark.parametrize("n_pad,n", [(256, 200), (768, 600), (2304, 2300)])
def test_random_inputs_within_slack(n_pad, n):
    rng = np.random.default_rng(n_pad)
    for _ in range(20):
        al, be = rng.uniform(-2, 2, 2)
        _check(_inputs(rng, n_pad, n, lambda r, k: 1.0) + (al, be))


@pytest.mark.parametrize("n_pad,n", [(256, 200), (768, 600), (2304, 2300)])
def test_wide_range_u_and_large_offsets(n_pad, n):
    """|alpha|, |beta| near 2 and U entries over 1e-8 .. 1e2: fp16 subnormals (below 6.1e-5, absolute
    error 2^-25) and normal roundings (2^-11 relative) in the same sums"""
    rng = np.random.default_rng(7 * n_pad)
    wide = lambda r, k: 10.0 ** r.uniform(-8, 2, k)
    for sa in (1, -1):
        for sb in (1, -1):
            for _ in range(5):
                al, be = sa * rng.uniform(1.9, 2.0), sb * rng.uniform(1.9, 2.0)
                _check(_inputs(rng, n_pad, n, wide) + (al, be))


def test_all_subnormal_u_is_covered_by_the_absolute_term():
    rng = np.random.default_rng(11)
    tiny = lambda r, k: np.full(k, 3e-6)
    for _ in range(10):
        _check(_inputs(rng, 768, 600, tiny) + (1.97, -1.93))


@pytest.mark.parametrize("n_pad,n", [(256, 200), (768, 600), (2304, 2300)])
@pytest.mark.parametrize("which", ["i", "j"])
def test_fp16_overflow_keeps_the_pair(n_pad, n, which):
    """a U entry past fp16's range reads as inf: the sums turn inf / NaN and the screen's test
    !(var_lo > 0) keeps the pair whatever w'Pw is"""
    rng = np.random.default_rng(13)
    a, b, ua, ub, z, dg, py = _inputs(rng, n_pad, n, lambda r, k: 1.0)
    a[5] = b[5] = 1.0
    (ua if which == "i" else ub)[5] = 1e5
    side, slack, eff, eff_slack, sw = pair_side(a, b, ua, ub, z, dg, py, 0.7, 1.1)
    for m_quad in (0.0, 1e30):
        var_lo = m_quad + side - slack
        assert not (var_lo > 0.0)
    # and with a zero code on the overflowing individual (0 x inf = NaN)
    a[5] = 0.0
    side, slack, *_ = pair_side(a, b, ua, ub, z, dg, py, 0.7, 1.1)
    assert not (1e30 + side - slack > 0.0)
