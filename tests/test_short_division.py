"""The baked traversal's short division and short normalisation (pdiv_short over prcp_core, normalize_short,
local_direction_lean: pine_amd/csrc/pine_math.h "division", pine_device.h) must give the bits of the
compiler's `n / d`, and of normalize() followed by prcp(), for every operand: inside the window by the short sequence,
outside it by the fallback.  pine_gpu_test_short_div runs both on the device and compares there; nothing here has a
tolerance.  Each test also pins WHICH form ran: the short one for exactly the operands inside the window."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIV_LO, DIV_HI = np.float32(2.0 ** -42), np.float32(2.0 ** 42)  # kDivLo, kDivHi
RAY_LO, RAY_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)  # kRayLo, kRayHi
E_LO, E_HI = 127 - 42, 127 + 42                                 # the biased exponents of the division window's ends


def _run(kind, gen, cases=None, p=(0, 0, 0), n=None, cap=8):
    from pine_amd import _lib
    stats = (C.c_int64 * 4)()
    ex = np.zeros((cap, 8), dtype=np.uint32)
    ptr = None
    if cases is not None:
        cases = np.ascontiguousarray(cases, dtype=np.uint32)
        n, ptr = len(cases), cases.ctypes.data_as(C.POINTER(C.c_uint32))
    _lib.check(_lib.lib.pine_gpu_test_short_div(0, kind, gen, ptr, p[0], p[1], p[2], n, stats, ex.ctypes.data_as(C.POINTER(C.c_uint32)), cap),
               "pine_gpu_test_short_div")
    cases_run, bad, taken, outside = (int(v) for v in stats)
    assert cases_run == n
    assert bad == 0, (kind, gen, p, bad, [[hex(w) for w in row] for row in ex[:min(bad, cap)]])
    assert outside == 0, (kind, gen, p, outside)  # (no operand outside the window ever took the short form)
    return taken


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _within(u, lo, hi):
    a = np.asarray(u, dtype=np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        return (np.abs(a) >= lo) & (np.abs(a) <= hi)


def _pairs(a, b):
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return np.stack([np.repeat(a, len(b)), np.tile(b, len(a))], axis=1)


def _edge_values(edge):
    """The window's end `edge` moved by -2 ... +2 exponents, each exactly and one ulp to either side, of either sign."""
    v = []
    for k in range(-2, 3):
        x = np.float32(edge * np.float32(2.0 ** k))
        v += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    v = np.float32(v)
    return _bits(np.concatenate([v, -v]))


RNG = np.random.default_rng(4242)
ORDINARY = _bits(np.concatenate([np.float32([1.0, -1.0, 3.0, 0.1, -555.0, 1.9, 2.0, float.fromhex("0x1.fffffep0"), float.fromhex("0x1.000002p0"), 1e-9, -7e11]),
                                 (RNG.uniform(1, 2, 12) * 2.0 ** RNG.integers(-41, 41, 12) * RNG.choice([-1, 1], 12)).astype(np.float32)]))
SPECIAL = np.uint32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00400000, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                     0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc01234, 0x7f800001, 0xff8abcde])


def test_every_denominator_mantissa():
    """All 2^23 mantissas of the denominator at six exponents across the window (both ends, their neighbours, the middle), each
    against a dozen numerators: mantissa all zeros, all ones, alternating bits, random; numerator exponents across the window;
    every combination of signs."""
    mant = [0x000000, 0x7fffff, 0x2aaaaa, 0x555555] + [int(m) for m in RNG.integers(0, 1 << 23, 8)]
    nexp = [E_LO, 127, E_HI - 1, E_LO + 1, 100, 150, 127, 128, E_HI - 1, E_LO, 126, 140]
    total = 0
    for j, dexp in enumerate([E_LO, E_LO + 1, 126, 127, 128, E_HI - 1]):
        for i, (m, e) in enumerate(zip(mant, nexp)):
            num = (((i >> 1) & 1) << 31) | (e << 23) | m
            den0 = (((i + j) & 1) << 31) | (dexp << 23)
            taken = _run(0, 1, p=(den0, num, 0), n=1 << 23)
            assert taken == 1 << 23, (hex(num), hex(den0), taken)  # (all of them inside the window: the short form ran)
            total += taken
    assert total == 72 << 23


def test_random_pairs_in_the_window():
    n = 1 << 26
    assert _run(0, 2, p=(20260, E_LO, E_HI - 1), n=n) == n
    # ... and pairs whose exponents reach four past either end: part of them fall back
    taken = _run(0, 2, p=(20261, E_LO - 4, E_HI + 4), n=1 << 22)
    assert 0.6 * (1 << 22) < taken < 0.95 * (1 << 22), taken


def test_window_edges_and_special_operands():
    """Pairs straddling each end of the window by +-2 exponents and +-1 ulp; zeros of both signs, denormals, the largest finite
    values, infinities and NaNs on either side.  The short form runs for exactly the pairs with both operands inside."""
    edges = np.concatenate([_edge_values(DIV_LO), _edge_values(DIV_HI)])
    every = np.concatenate([edges, ORDINARY, SPECIAL])
    cases = np.concatenate([_pairs(edges, every), _pairs(every, edges), _pairs(SPECIAL, every), _pairs(every, SPECIAL)])
    inside = _within(cases[:, 0], DIV_LO, DIV_HI) & _within(cases[:, 1], DIV_LO, DIV_HI)
    assert 0.1 < inside.mean() < 0.9
    assert _run(0, 0, cases) == int(inside.sum())
    # one case at a time at the very ends: 2^-42 and 2^42 are inside, their neighbours towards zero / infinity are not
    for x, want in ((DIV_LO, 1), (np.nextafter(DIV_LO, np.float32(0)), 0), (DIV_HI, 1), (np.nextafter(DIV_HI, np.float32(np.inf)), 0), (np.float32(0), 0)):
        for s in (1, -1):
            one = _bits([np.float32(s) * x])[0]
            assert _run(0, 0, [[one, _bits([3.0])[0]]]) == want and _run(0, 0, [[_bits([-3.0])[0], one]]) == want, (x, s)


def test_short_normalize():
    """local_direction_lean (the direction and the reciprocals of its components) against normalize() and prcp(): 2^22 random
    vectors; vectors with one or two components at, just above and just below the window's floor and ceiling, zero or denormal;
    vectors along the axes; components that are not finite."""
    n = 1 << 22
    taken = _run(1, 2, p=(777, 127 - 40, 127 + 39), n=n)
    assert taken == n
    taken = _run(1, 2, p=(778, 127 - 44, 127 + 44), n=n)  # (exponents past both ends: about a quarter fall back)
    assert 0.6 * n < taken < 0.9 * n, taken
    floor = np.float32([RAY_LO, np.nextafter(RAY_LO, np.float32(1)), np.nextafter(RAY_LO, np.float32(0)), RAY_LO * 2, RAY_LO / 2, RAY_LO / 4,
                        0.0, 1e-40, 1.1754944e-38, RAY_HI, np.nextafter(RAY_HI, np.float32(0)), np.nextafter(RAY_HI, np.float32(np.inf)), RAY_HI * 2])
    floor = np.concatenate([floor, -floor])
    rng = np.random.default_rng(31)
    per = 4000
    vecs = []
    for count in (1, 2, 3):
        v = (rng.normal(size=(per, 3)) * 2.0 ** rng.integers(-30, 30, (per, 1))).astype(np.float32)
        mask = np.argsort(rng.random((per, 3)), axis=1) < count
        vecs.append(np.where(mask, rng.choice(floor, (per, 3)), v))
    axes = []
    for a in (1.0, -1.0, 3.7, RAY_LO, RAY_HI, 1e-30, 1e30, 0.0):
        for k in range(3):
            for other in (0.0, -0.0, float(RAY_LO), float(np.nextafter(RAY_LO, np.float32(0)))):
                v = np.full(3, other, dtype=np.float32)
                v[k] = a
                axes.append(v)
    vecs.append(np.float32(axes))
    odd = SPECIAL.view(np.float32)
    v = rng.normal(size=(per, 3)).astype(np.float32)
    vecs.append(np.where(np.argsort(rng.random((per, 3)), axis=1) < 1, rng.choice(odd, (per, 3)), v))
    cases = _bits(np.concatenate(vecs))
    inside = _within(cases, RAY_LO, RAY_HI).all(axis=1)
    assert 0.05 < inside.mean() < 0.9, inside.mean()
    assert _run(1, 0, cases) == int(inside.sum())
