"""The scalar functions every path kernel inlines -- psqrt, prcp (pine_math.h's guarded short forms), psin / pcos / psincos,
plog, pacos, patan2, ppow (pine_libm.h's glibc restatements), division and pmin / pmax / pclamp -- over their input domains,
bit for bit against a reference: the host's correctly rounded IEEE sqrtf / 1.0f / x / x / y, the host's glibc (the libm the
reference links), or the same comparison expressions on the host (include/pine_gpu.h, pine_gpu_test_math_*).

CPU: the comparator reports each kind of error with its input; the host build of the same functions (device = -1) passes
strided sweeps of every function and the edge-value sets.
GPU: the device build, compiled with the path kernels' flags in pine_test_hooks.hip: all 2^32 arguments of the one-argument
functions and of powf(x, 5) (Schlick), strided sweeps of the two-argument ones at fixed special values, the edge-value
cross products, and random division pairs."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

FN = dict(sqrt=0, rcp=1, sin=2, cos=3, sincos=4, log=5, acos=6, atan2=7, pow=8, div=9, min=10, max=11, clamp=12)
ARITY = dict(sqrt=1, rcp=1, sin=1, cos=1, sincos=1, log=1, acos=1, atan2=2, pow=2, div=2, min=2, max=2, clamp=3)
WIDTH = dict((k, 2 if k == "sincos" else 1) for k in FN)
ALL = 1 << 32


def f32(*vals):
    return np.float32(vals).view(np.uint32)


def u32(*bits):
    return np.array(bits, dtype=np.uint32)


# ~60 values where scalar kernels go wrong: signed zeros, denormals, the normal boundary, 1 and its neighbours, the largest
# finite values, infinities, NaNs (quiet, negative, signalling payload), and magnitudes whose quotients and products
# overflow or underflow
EDGE_POSITIVE = np.concatenate([
    u32(0x00000000, 0x00000001, 0x00000002, 0x00000003, 0x00400000, 0x007fffff,  # 0, denormals
        0x00800000, 0x00800001, 0x01000000,                                       # min normal and up
        0x3f7fffff, 0x3f800000, 0x3f800001, 0x7f7ffffe, 0x7f7fffff, 0x7f800000),  # 1 -+ ulp, FLT_MAX, inf
    f32(0.5, 2.0, 3.0, 0.7, 1.5, np.pi, 2.0 ** 64, 2.0 ** -64, 2.0 ** 100, 2.0 ** -100, 2.0 ** 127, 2.0 ** -126 * 1.5,
        1.0e10, 1.0e-10, 3.0e38, 2.0 ** 24 + 1),
])
EDGE = np.unique(np.concatenate([EDGE_POSITIVE, EDGE_POSITIVE | np.uint32(0x80000000),
                                 u32(0x7fc00000, 0xffc00000, 0x7fa00000)]))


class Result:
    def __init__(self, label, stats, examples, fn):
        self.label, self.fn = label, fn
        self.checked, self.mismatches, self.nan_payload_only, self.max_ulp = (int(v) for v in stats)
        self.examples = [tuple(int(w) for w in e) for e in examples[: min(self.mismatches, len(examples))]]

    def __str__(self):
        def show(u):
            return f"{u:08x} ({np.uint32(u).view(np.float32)!r})"
        text = (f"{self.label}: checked {self.checked}, mismatches {self.mismatches}, nan payload only "
                f"{self.nan_payload_only}, max ulp {self.max_ulp}")
        for a, b, c, got, want in self.examples:
            args = ", ".join(show(v) for v in (a, b, c)[: ARITY[self.fn]])
            which = ("sin", "cos")[b] + " " if self.fn == "sincos" else ""
            text += f"\n    {self.fn}({args}): {which}got {show(got)}, want {show(want)}"
        return text


def _p32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def sweep(device, fn, fixed=0, swept=0, first=0, count=ALL, stride=1, cap=8):
    from pine_amd import _lib
    assert stride % 2 == 1, "an odd stride reaches every residue: each binade and both signs"
    stats = np.zeros(4, np.int64)
    ex = np.zeros((cap, 5), np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_math_sweep(device, FN[fn], int(fixed), swept, int(first) & 0xffffffff, count, stride,
                                                 stats.ctypes.data_as(C.POINTER(C.c_int64)), _p32(ex), cap),
               "pine_gpu_test_math_sweep")
    label = f"{'host' if device < 0 else 'device'} {fn} sweep arg {swept} from {int(first):08x} x {count} / {stride}"
    if ARITY[fn] > 1:
        label += f", others {int(fixed):08x} ({np.uint32(fixed).view(np.float32)!r})"
    return Result(label, stats, ex, fn)


def evaluate(device, fn, a, b=None, c=None):
    from pine_amd import _lib
    a, b, c = (None if v is None else np.ascontiguousarray(v, np.uint32) for v in (a, b, c))
    got = np.zeros(a.size * WIDTH[fn], np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_math_eval(device, FN[fn], _p32(a), _p32(b), _p32(c), a.size, _p32(got)),
               "pine_gpu_test_math_eval")
    return got


def compare(fn, got, a, b=None, c=None, cap=8, label=""):
    from pine_amd import _lib
    a, b, c = (None if v is None else np.ascontiguousarray(v, np.uint32) for v in (a, b, c))
    stats = np.zeros(4, np.int64)
    ex = np.zeros((cap, 5), np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_math_compare(FN[fn], _p32(a), _p32(b), _p32(c), _p32(np.ascontiguousarray(got)), a.size,
                                                   stats.ctypes.data_as(C.POINTER(C.c_int64)), _p32(ex), cap),
               "pine_gpu_test_math_compare")
    return Result(label or f"{fn} on {a.size} arguments", stats, ex, fn)


def check_clean(r, checked=None):
    print(r)
    assert r.mismatches == 0, str(r)
    if checked is not None:
        assert r.checked == checked, str(r)


def edge_product(arity):
    cols = np.array(list(itertools.product(range(EDGE.size), repeat=arity)), dtype=np.int64).T
    return [EDGE[k] for k in cols]


# ---- the comparator (CPU) ----------------------------------------------------------------------------------------
def test_comparator_reports_each_kind_of_error_with_its_input():
    rng = np.random.default_rng(3)
    a = np.concatenate([EDGE, rng.integers(0, ALL, 4000, dtype=np.uint64).astype(np.uint32)])
    b = np.roll(a, 7)
    c = np.roll(a, 31)
    for fn in ("sqrt", "sin", "sincos", "pow", "div", "clamp"):
        args = [a, b, c][: ARITY[fn]]
        got = evaluate(-1, fn, *args)
        r = compare(fn, got, *args)
        check_clean(r, a.size * WIDTH[fn])
        w = WIDTH[fn]
        res = got.reshape(-1, w)[:, 0]
        finite = np.flatnonzero(((res & 0x7fffffff) > 0) & ((res & 0x7fffffff) < 0x7f000000))
        nan = np.flatnonzero((res & 0x7fffffff) > 0x7f800000)
        zero = np.flatnonzero((res & 0x7fffffff) == 0)

        def corrupt(i, value):
            bad = got.copy()
            bad[i * w] = value
            r = compare(fn, bad, *args, label=f"{fn} with result {i} corrupted")
            print(r)
            return r

        def expect_reported(r, i, value, ulp):
            assert (r.mismatches, r.nan_payload_only) == (1, 0), str(r)
            want_args = tuple(int(v[i]) for v in args) + (0,) * (3 - len(args))
            if w == 2:  # SINCOS: b names the output
                want_args = (want_args[0], 0, want_args[2])
            assert r.examples == [want_args + (int(value), int(got[i * w]))], str(r)
            if ulp is not None:
                assert r.max_ulp == ulp, str(r)

        i = int(finite[len(finite) // 2])
        expect_reported(corrupt(i, got[i * w] + 1), i, got[i * w] + 1, 1)  # one ulp
        i = int(zero[0])
        expect_reported(corrupt(i, got[i * w] ^ 0x80000000), i, got[i * w] ^ 0x80000000, 1)  # the other zero
        i = int(finite[0])
        expect_reported(corrupt(i, 0x7fc00000), i, 0x7fc00000, 0)  # NaN for a number (no ulp distance)
        if len(nan):
            i = int(nan[0])
            expect_reported(corrupt(i, 0x3f800000), i, 0x3f800000, 0)  # a number for NaN
            r = corrupt(i, got[i * w] ^ 0x80400001)  # another NaN: counted apart, not a mismatch
            assert (r.mismatches, r.nan_payload_only) == (0, 1), str(r)
        # several errors: the first `cap` in input order
        bad = got.copy()
        idx = np.sort(rng.choice(finite, 5, replace=False))
        bad[idx * w] ^= 1
        r = compare(fn, bad, *args, cap=3)
        assert r.mismatches == 5 and [e[0] for e in r.examples] == [int(a[k]) for k in idx[:3]], str(r)


def test_comparator_checks_both_results_of_sincos():
    a = f32(0.5, 200.0, -1.0e30)
    got = evaluate(-1, "sincos", a)
    bad = got.copy()
    bad[3] ^= 2  # cos(200)
    r = compare("sincos", bad, a)
    print(r)
    assert r.checked == 6 and r.mismatches == 1 and r.max_ulp == 2
    assert r.examples == [(int(a[1]), 1, 0, int(bad[3]), int(got[3]))]


def test_sweep_generates_the_arguments_it_reports():
    from pine_amd import PineError
    # x = first + k * stride (mod 2^32) for k < count; a wrong result names its x and the fixed argument
    r = sweep(-1, "div", fixed=f32(3.0)[0], swept=0, first=0xfffffff0, count=100, stride=0x10001)
    check_clean(r, 100)
    r = sweep(-1, "clamp", fixed=f32(-1.0)[0], swept=2, first=5, count=3, stride=1)
    check_clean(r, 3)
    with pytest.raises(PineError):
        sweep(-1, "sqrt", swept=1, count=10)
    with pytest.raises(PineError):
        sweep(-1, "sqrt", count=ALL + 1)


# ---- the host build of the same functions (CPU) ---------------------------------------------------------------------
@pytest.mark.parametrize("fn", list(FN))
def test_host_build_sweeps(fn):
    """device = -1: every function strided over all bit patterns of each argument (the other ones fixed at values of the
    edge set), then the edge-set cross product.  The sine / cosine sweeps cover |x| >= 120, the large-argument path."""
    t0 = time.perf_counter()
    if ARITY[fn] == 1:
        check_clean(sweep(-1, fn, first=0x1234567, count=ALL // 251 + 1, stride=251))
    else:
        for swept in range(ARITY[fn]):
            for fixed in f32(-2.0, -0.5, 0.0, 1.0, 2.2, 1.0e10)[:: (1 if ARITY[fn] == 2 else 2)]:
                check_clean(sweep(-1, fn, fixed=fixed, swept=swept, first=0x89abcdef, count=ALL // 4099 + 1, stride=4099))
    args = edge_product(ARITY[fn])
    check_clean(compare(fn, evaluate(-1, fn, *args), *args, label=f"host {fn} on the edge set"))
    print(f"{fn}: {time.perf_counter() - t0:.1f} s")


# ---- the device build (GPU) -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def glibc():
    libc = C.CDLL("libc.so.6")
    libc.gnu_get_libc_version.restype = C.c_char_p
    version = libc.gnu_get_libc_version().decode()
    print(f"reference: the host's glibc {version}")
    return version


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["sqrt", "rcp", "sin", "cos", "sincos", "log", "acos"])
def test_device_one_argument_functions_on_every_float(fn, glibc):
    t0 = time.perf_counter()
    check_clean(sweep(0, fn), ALL * WIDTH[fn])
    print(f"{fn}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
def test_device_pow_schlick_on_every_float(glibc):
    t0 = time.perf_counter()
    check_clean(sweep(0, "pow", fixed=f32(5.0)[0], swept=0), ALL)
    print(f"pow(x, 5): {time.perf_counter() - t0:.1f} s")


STRIDE = 65  # odd; 2^32 / 65 = 66 million arguments per sweep


@pytest.mark.gpu
def test_device_pow_strided_sweeps(glibc):
    t0 = time.perf_counter()
    ys = f32(2.0, 3.0, 0.5, 2.2, 1 / 2.2, -1.0, -2.0, -0.5, 0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 2.0 ** 24 + 1,
             1.0e10, -1.0e10)
    ys = np.concatenate([ys, u32(0x00000001)])  # 2^-149
    for y in ys:
        check_clean(sweep(0, "pow", fixed=y, swept=0, first=int(y) * 7, count=ALL // STRIDE + 1, stride=STRIDE))
    xs = f32(-2.0, -1.0, -0.5, 0.0, -0.0, 0.5, 1.0, 2.0, np.inf, -np.inf, np.nan, 3.4028234663852886e38)
    xs = np.concatenate([xs, u32(0x00000001)])
    for x in xs:
        check_clean(sweep(0, "pow", fixed=x, swept=1, first=int(x) * 7, count=ALL // STRIDE + 1, stride=STRIDE))
    args = edge_product(2)
    check_clean(compare("pow", evaluate(0, "pow", *args), *args, label="device pow on the edge set"))
    print(f"pow sweeps: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
def test_device_atan2_strided_sweeps(glibc):
    t0 = time.perf_counter()
    fixed = np.concatenate([f32(1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 0.7, 3.0e38), u32(0x00000001)])
    for swept in (0, 1):  # y swept at fixed x, then x swept at fixed y
        for v in fixed:
            check_clean(sweep(0, "atan2", fixed=v, swept=swept, first=int(v) * 7, count=ALL // STRIDE + 1, stride=STRIDE))
    args = edge_product(2)
    check_clean(compare("atan2", evaluate(0, "atan2", *args), *args, label="device atan2 on the edge set"))
    print(f"atan2 sweeps: {time.perf_counter() - t0:.1f} s")


def log_uniform_pairs(n, seed):
    # every biased exponent (denormals included) equally likely, random mantissas and signs
    rng = np.random.default_rng(seed)
    bits = [(rng.integers(0, 255, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
            | (rng.integers(0, 2, n, dtype=np.uint32) << 31) for _ in range(2)]
    return bits


@pytest.mark.gpu
def test_device_division(glibc):
    t0 = time.perf_counter()
    a, b = edge_product(2)
    check_clean(compare("div", evaluate(0, "div", a, b), a, b, label="device a / b on the edge set"), a.size)
    a, b = log_uniform_pairs(10_000_000, 11)
    check_clean(compare("div", evaluate(0, "div", a, b), a, b, label="device a / b on random pairs"), a.size)
    # quotients near overflow and underflow: b in [2^-127, 2^-125] and [2^125, 2^127]
    for lo in (0x00400000, 0x7e000000):
        check_clean(sweep(0, "div", fixed=f32(3.0)[0], swept=1, first=lo, count=0x01000000 // 3 * 3, stride=3))
    print(f"division: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["min", "max", "clamp"])
def test_device_comparisons_on_the_edge_set(fn, glibc):
    args = edge_product(ARITY[fn])
    check_clean(compare(fn, evaluate(0, fn, *args), *args, label=f"device {fn} on the edge set"), args[0].size)
