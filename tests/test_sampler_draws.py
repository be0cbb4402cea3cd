"""SobolSampler, HaltonSampler and BlueSampler draws per call, at the film sizes, sample counts and indices people render with:
the kernels' sampler front (sampler_get1d / sampler_get2d, pine_device.h) through pine_gpu_test_sampler_draws, whose tables come
from the code that builds a plan's, against what the REAL reference's sampler objects returned (`pine_ref draws`,
tests/golden/sampler_draws_*.npz: tools/make_golden.py --draws; the case tables are inside the fixtures).  Bit patterns only.

CPU: the host build of the same functions, the oracle's sampler object (what every oracle.render(..., sampler=...) comparison
rests on), the derived Halton tables against the reference's, oracle.render on the strip films.
GPU (-m gpu): the gfx950 build of the functions, from memory and through the LDS cache of a 256-thread workgroup; the strip
films -- pixel coordinates past 128 and past a 512 Morton range -- through both path kernels."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal, load_film
from strip_scenes import STRIP_FILM_NAMES, strip_scene

KIND_NAMES = {0: "blue", 1: "sobol", 2: "halton"}
_fixture_cache = {}


def fixture(name):
    """(cases[n,9] int32, draws float32, first float of each case, the npz) of tests/golden/sampler_draws_<name>.npz, read once."""
    if name not in _fixture_cache:
        from oracle.oracle import draw_floats
        z = np.load(os.path.join(GOLDEN, f"sampler_draws_{name}.npz"))
        cases, draws = np.ascontiguousarray(z["cases"], np.int32), z["draws"]
        offsets = np.concatenate([[0], np.cumsum(draw_floats(cases))])
        assert cases.shape[1] == 9 and offsets[-1] == draws.size
        cases.setflags(write=False), draws.setflags(write=False)
        _fixture_cache[name] = (cases, draws, offsets, z)
    return _fixture_cache[name]


def groups():
    """Every (fixture, kind, w, h, spp) of the fixtures, with the rows of its cases: one call of the hook each."""
    out = []
    for name in ("sobol", "halton"):
        cases = fixture(name)[0]
        keys = list(dict.fromkeys(map(tuple, cases[:, [0, 2, 3, 1]].tolist())))
        out += [(name, k, w, h, spp) for k, w, h, spp in keys]
    return out


GROUPS = groups()
GROUP_IDS = [f"{KIND_NAMES[k]}-{w}x{h}-s{spp}" for _, k, w, h, spp in GROUPS]


def group_rows(name, kind, w, h, spp):
    cases = fixture(name)[0]
    return np.flatnonzero((cases[:, [0, 2, 3, 1]] == (kind, w, h, spp)).all(axis=1))


def expected(name, rows):
    _, draws, offsets, _ = fixture(name)
    return np.concatenate([draws[offsets[r]:offsets[r + 1]] for r in rows])


def describe_first_difference(name, rows, got):
    """None, or the first differing float's case: pixel, sample index, call number, dimension."""
    cases, _, offsets, _ = fixture(name)
    want = expected(name, rows)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if bad.size == 0:
        return None
    at, start = int(bad[0]), 0
    for r in rows:
        n = int(offsets[r + 1] - offsets[r])
        if at < start + n:
            kind, spp, w, h, px, py, index, pattern, calls = cases[r].tolist()
            # replay the dimension counter: SobolSampler's runs on, HaltonSampler's wraps to 2 at 1000, BlueSampler's at 256
            wrap = {0: 256, 1: None, 2: 1000}[kind]
            dim, k = (2 if kind == 2 else 0), start
            for call in range(calls):
                width = 1 if pattern == 2 or (pattern == 1 and call % 2 == 0) else 2
                if wrap and dim + width - 1 >= wrap:
                    dim = 2
                if at < k + width:
                    return (f"{bad.size} of {want.size} floats differ; first: {KIND_NAMES[kind]} spp {spp} film {w}x{h} pixel ({px}, {py}) sample {index} "
                            f"pattern {pattern} call {call} ({'get1d' if width == 1 else 'get2d'}) dimension {dim + at - k}: "
                            f"{got[at]!r} ({got.view(np.uint32)[at]:#010x}) instead of {want[at]!r} ({want.view(np.uint32)[at]:#010x})")
                dim, k = dim + width, k + width
        start += n
    return f"{bad.size} of {want.size} floats differ; first at float {at}"


def hook_draws(device, name, kind, w, h, spp, mode=0):
    from pine_amd import _lib
    rows = group_rows(name, kind, w, h, spp)
    cases = np.ascontiguousarray(fixture(name)[0][rows])
    out = np.full(expected(name, rows).size, np.nan, np.float32)
    n = _lib.check(_lib.lib.pine_gpu_test_sampler_draws(device, kind, spp, w, h, mode, cases.ctypes.data_as(C.POINTER(C.c_int32)), len(cases),
                                                        out.ctypes.data_as(_lib.c_f_p), out.size), "pine_gpu_test_sampler_draws")
    assert n == out.size
    return rows, out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_the_fixtures_hold_the_cases_they_are_for():
    """What the case tables must reach (the rest of this module reads them from the files): Morton codes of coordinates above
    63, Sobol indices up to 2^44, both parities of log2(spp), a count that is no power of two; Halton pixels on both sides
    of 128, the last index the device takes, streams past the 1000-prime wrap twice; Blue pixels on both sides of 128."""
    sobol = fixture("sobol")[0]
    s = sobol[sobol[:, 0] == 1]
    assert {(45, 37, 12), (64, 64, 1), (1920, 1080, 2), (1920, 1080, 1024), (65535, 1, 4096), (1, 65535, 8)} <= set(map(tuple, s[:, [2, 3, 1]].tolist()))
    assert ((s[:, 4] == 65534) & (s[:, 1] == 4096) & (s[:, 6] == 4095)).any() and ((s[:, 5] == 65534) & (s[:, 6] == 7)).any()
    for w, h, spp in set(map(tuple, s[:, [2, 3, 1]].tolist())):
        g = s[(s[:, [2, 3, 1]] == (w, h, spp)).all(axis=1)]
        corners, pixels = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}, set(map(tuple, g[:, 4:6].tolist()))
        assert corners < pixels  # (and an interior pixel)
        assert {0, spp // 2, spp - 1} == set(g[:, 6].tolist()) and {0, 1} == set(g[:, 7].tolist()) and (g[:, 8] >= 100).all()
    b = sobol[sobol[:, 0] == 0]
    assert {1, 16, 256} == set(b[:, 1].tolist()) and (b[:, 4] < 128).any() and (b[:, 4] >= 128).any() and (b[:, 5] >= 128).any()
    hal = fixture("halton")[0]
    assert (hal[:, 0] == 2).all() and (hal[:, 1] == 4096).all()
    assert {(0, 0), (127, 127), (128, 5), (129, 242), (1919, 1079), (65534, 0)} == set(map(tuple, hal[:, 4:6].tolist()))
    for pattern, indices, dims in ((0, {0, 1, 4095}, 1000), (1, {0, 1, 4095}, 2 * 998 + 2), (2, {4095}, 1000)):
        g = hal[hal[:, 7] == pattern]
        assert indices <= set(g[:, 6].tolist())
        floats = g[:, 8] * 2 if pattern == 0 else g[:, 8] + g[:, 8] // 2 if pattern == 1 else g[:, 8]
        assert (floats >= dims).all()  # (from dimension 2: past 1000 once; the alternating pattern twice, on a get2d and on a get1d)


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_host_build_of_the_sampler_front_equals_the_reference(group):
    rows, got = hook_draws(-1, *group)
    assert (why := describe_first_difference(group[0], rows, got)) is None, why


def test_halton_tables_equal_the_reference():
    """The primes, their prefix sums and the 3 682 913 digit permutations the library derives (halton_host_tables) against the
    CRC-32 of the reference's Primes, PrimeSums and HaltonSampler::radicalInversePermutations."""
    from pine_amd import _lib
    z = fixture("halton")[3]
    crc, counts = np.zeros(3, np.uint32), np.zeros(3, np.int64)
    _lib.check(_lib.lib.pine_gpu_test_halton_tables(crc.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data_as(C.POINTER(C.c_int64))),
               "pine_gpu_test_halton_tables")
    assert counts.tolist() == z["table_counts"].tolist() == [1000, 1000, 3682913]
    assert crc.tolist() == z["table_crc32"].tolist()
    # (the hook's CRC-32 is zlib's, as the fixture's: the two small tables once more, from primes found here)
    primes = [n for n in range(2, 8000) if all(n % d for d in range(2, int(n ** 0.5) + 1))][:1000]
    assert crc[0] == zlib.crc32(np.int32(primes).tobytes()) and crc[1] == zlib.crc32(np.int32(np.cumsum([0] + primes[:-1])).tobytes())


@pytest.mark.parametrize("name", ["sobol", "halton"])
def test_oracle_sampler_equals_the_reference(oracle, name):
    """The oracle's sampler object -- the one oracle.render draws from -- on every case: what makes it a yardstick for the
    SobolSampler / HaltonSampler comparisons of films wider than the 48 pixels of the reference's films."""
    cases = fixture(name)[0]
    got = oracle.sampler_draws(cases)
    assert (why := describe_first_difference(name, np.arange(len(cases)), got)) is None, why


def test_bad_arguments_are_refused_before_anything_runs():
    from pine_amd import _lib
    out = np.zeros(4096, np.float32)

    def call(kind, spp, w, h, mode, case, capacity=out.size, device=-1):
        q = np.int32([case])
        return _lib.lib.pine_gpu_test_sampler_draws(device, kind, spp, w, h, mode, q.ctypes.data_as(C.POINTER(C.c_int32)), 1, out.ctypes.data_as(_lib.c_f_p), capacity)

    good = [1, 64, 100, 50, 99, 49, 63, 1, 10]
    assert call(1, 64, 100, 50, 0, good) == 15
    for why, args in (("samples per pixel must be positive", (1, 0, 100, 50, 0, [1, 0, 100, 50, 0, 0, 0, 0, 1])),
                      ("at most 4096 samples per pixel", (1, 4097, 100, 50, 0, [1, 4097, 100, 50, 0, 0, 0, 0, 1])),
                      ("a film side is 1 .. 65535 pixels", (1, 64, 65536, 50, 0, [1, 64, 65536, 50, 0, 0, 0, 0, 1])),
                      ("a film side is 1 .. 65535 pixels", (2, 64, 100, 0, 0, [2, 64, 100, 0, 0, 0, 0, 0, 1])),
                      ("pixel lies outside the film", (1, 64, 100, 50, 0, [1, 64, 100, 50, 100, 49, 0, 0, 1])),
                      ("pixel lies outside the film", (1, 64, 100, 50, 0, [1, 64, 100, 50, 0, -1, 0, 0, 1])),
                      ("sample index lies outside", (1, 64, 100, 50, 0, [1, 64, 100, 50, 0, 0, 64, 0, 1])),
                      ("sample index lies outside", (0, 5, 100, 50, 0, [0, 5, 100, 50, 0, 0, 8, 0, 1])),  # (BlueSampler(5) has 8 samples)
                      ("another sampler or film", (1, 64, 100, 50, 0, [2, 64, 100, 50, 0, 0, 0, 0, 1])),
                      ("pattern is 0, 1 or 2", (1, 64, 100, 50, 0, [1, 64, 100, 50, 0, 0, 0, 3, 1])),
                      ("calls at most 65536", (1, 64, 100, 50, 0, [1, 64, 100, 50, 0, 0, 0, 0, 65537])),
                      ("bad argument", (3, 64, 100, 50, 0, [3, 64, 100, 50, 0, 0, 0, 0, 1])),
                      ("bad argument", (1, 64, 100, 50, 2, good)),
                      ("the LDS form runs on the device only", (0, 16, 100, 50, 1, [0, 16, 100, 50, 0, 0, 0, 0, 1]))):
        assert call(*args) < 0 and why in _lib.last_error(), (why, _lib.last_error())
    assert call(1, 64, 100, 50, 0, good, capacity=14) < 0 and "capacity too small" in _lib.last_error()


@pytest.mark.parametrize("name", STRIP_FILM_NAMES)
def test_oracle_renders_the_strip_films(oracle, name):
    ref, ps, spp, depth = load_film(name)
    scene, sampler, s, d = strip_scene(name)
    assert scene.describe() == ps and (s, d) == (spp, depth)
    h, w = ref.shape[:2]
    film, _ = oracle.render(ps, (w, h), spp, depth, sampler=sampler)
    assert_bit_equal(film, ref, name)
    # the strip is lit where the sampler's state matters: pixels past 128 (and the slit past 512) carry paths that drew from it
    lit = (ref[..., :3] != 0).any(axis=2)
    if "2x600" in name or "_slit_" in name:
        assert lit[:, 128:].any() if w > h else lit[128:].any()
        assert lit.mean() > 0.8


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["memory", "lds"])
@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_device_sampler_front_equals_the_reference(group, mode):
    """The gfx950 build: 64-bit shifts and multiplies, float(uint64), 32-bit division by a run-time prime, 1.0f / float(base)
    without contraction, v_bfrev_b32, 16-bit permutation reads 3.6 M entries into the table.  mode `memory`: MODE = 0
    (BlueSampler) or kSmSobol; `lds`: the same with kSmLds, the form the megakernel and the AO kernel instantiate."""
    rows, got = hook_draws(0, *group, mode=mode)
    assert (why := describe_first_difference(group[0], rows, got)) is None, why


@pytest.fixture(params=["queue", "mega"])
def path_kernel(request, monkeypatch):
    """Both path kernels, as tests/test_gpu_parity.py runs them."""
    if request.param == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    else:
        monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRIP_FILM_NAMES)
def test_strip_films_match_the_reference(name, path_kernel):
    import pine_amd as pa
    from test_gpu_parity import _render
    ref, ps, spp, depth = load_film(name)
    scene, sampler, _, _ = strip_scene(name)
    assert scene.describe() == ps
    film, st = _render(scene, pa.HaltonSampler(spp) if sampler == "halton" else pa.SobolSampler(spp), depth)
    assert st.block_threads == (1024 if path_kernel == "queue" else 256)  # the kernel under test is the one that ran
    assert st.spp_effective == spp
    assert_bit_equal(film, ref, f"{name} ({path_kernel})")
