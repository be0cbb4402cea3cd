"""Rendering in sample passes (pine_gpu_plan_create_passes): the pass planner on the host, and on the GPU the running
film -- the last pass leaves the reference's film bit for bit, every intermediate film is the partial sum it claims to be,
and the sample / checkpoint buffers are those of one pass.  Tolerance everywhere: zero."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import (EMBREE_FILM_NAMES, EMBREE_MORE_FILM_NAMES, FILM_NAMES, GOLDEN, HALTON_FILM_NAMES, SOBOL_FILM_NAMES,
                      assert_bit_equal, embree_scene, load_film)
from film_scenes import film_scene


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the planner
# ---------------------------------------------------------------------------------------------------------------------
def _schedule(w, h, rank, world, spp, k, serial, P):
    from pine_amd import _lib
    n = _lib.lib.pine_gpu_pass_schedule(w, h, rank, world, spp, k, serial, P, None, 0)
    assert n >= 1, _lib.last_error()
    out = (C.c_int32 * (4 * n))()
    assert _lib.lib.pine_gpu_pass_schedule(w, h, rank, world, spp, k, serial, P, out, 4 * n) == n
    return np.array(out[:], dtype=np.int64).reshape(n, 4)


def _local_tiles(w, h, rank, world):
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    return (tiles - rank + world - 1) // world


def _effective_p(spp, k, free, P):
    """The issue's rule: pass_samples clamped to [1, spp] (<= 0: spp), rounded down to a multiple of k (at least k) when the
    independent class has tiles."""
    p = spp if P <= 0 or P >= spp else P
    return max(k, p // k * k) if free > 0 else p


@pytest.mark.parametrize("size", [(1, 1), (45, 37), (640, 640), (1920, 1080)])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_pass_schedule_covers_every_tile_and_sample_row_once(size, world):
    w, h = size
    small = w * h <= 45 * 37
    for rank in range(world):
        tiles = _local_tiles(w, h, rank, world)
        for spp in (1, 2, 8, 12, 16, 64, 256, 1024, 4096):
            for k in sorted({1, 2, 4, spp}):
                if k > spp or spp % k:
                    continue
                for serial in sorted({0, tiles // 3, tiles}):
                    whole = tiles if k == spp else serial
                    free = tiles - whole
                    for P in sorted({1, 3, 5, k, max(1, spp // 4), max(1, spp // 2), max(1, spp - 1), spp, spp + 7, 0}):
                        s = _schedule(w, h, rank, world, spp, k, serial, P)
                        pe = _effective_p(spp, k, free, P)
                        n = -(-spp // pe)
                        assert len(s) == n, (size, world, rank, spp, k, serial, P)
                        # within a pixel of the independent class: increasing, contiguous sample ranges that end at spp,
                        # each a whole number of items
                        assert s[0, 0] == 0 and (s[1:, 0] == s[:-1, 0] + s[:-1, 1]).all() and s[-1, 0] + s[-1, 1] == spp
                        assert (s[:, 1] >= 1).all() and (s[:, 1] <= pe).all()
                        if free > 0:
                            assert (s[:, 0] % k == 0).all() and (s[:, 1] % k == 0).all()
                        # the whole-pixel tiles: contiguous slices of ceil(whole / n) that end at `whole`
                        per = -(-whole // n)
                        assert s[0, 2] == 0 and (s[1:, 2] == s[:-1, 2] + s[:-1, 3]).all() and s[-1, 2] + s[-1, 3] == whole
                        assert (s[:, 3] >= 0).all() and (s[:, 3] <= per).all()
                        # no pass holds more rows than tiles x P, plus one slice's rounding (ceil(whole / n) * spp <= whole * P + spp)
                        rows = s[:, 3] * spp + free * s[:, 1]
                        assert (rows <= tiles * pe + spp).all(), (size, world, rank, spp, k, serial, P, rows.max())
                        if small and spp <= 64:  # ... and, counted one by one, every (tile, sample row) exactly once
                            count = np.zeros((tiles, spp), np.int32)
                            for s0, ns, t0, nt in s:
                                count[t0:t0 + nt, :] += 1
                                count[whole:, s0:s0 + ns] += 1
                            assert (count == 1).all()


def test_pass_schedule_keeps_the_index_bound_where_one_launch_cannot():
    """3840 x 2160 at 1024 spp: tiles x 64 x spp is beyond 2^32; with 16 samples per pass every pass is far below."""
    tiles = _local_tiles(3840, 2160, 0, 1)
    assert tiles * 64 * 1024 >= 2 ** 32
    s = _schedule(3840, 2160, 0, 1, 1024, 2, 0, 16)
    assert len(s) == 64
    rows = s[:, 3] * 1024 + tiles * s[:, 1]
    assert ((rows + s[:, 0]) * 64 < 2 ** 32).all()
    # whole-pixel items only (a SobolSampler count that is not a power of two): slices of tiles
    s = _schedule(3840, 2160, 0, 1, 1000, 1000, 0, 16)
    assert len(s) == 63 and ((s[:, 3] * 1000) * 64 < 2 ** 32).all() and s[:, 3].sum() == tiles


def test_pass_schedule_rejects_bad_arguments():
    from pine_amd import _lib
    out = (C.c_int32 * 8)()
    for args in [(0, 8, 0, 1, 4, 1, 0, 2), (8, 8, 1, 1, 4, 1, 0, 2), (8, 8, 0, 1, 0, 1, 0, 2), (8, 8, 0, 1, 4, 3, 0, 2), (8, 8, 0, 1, 4, 1, 2, 2)]:
        assert _lib.lib.pine_gpu_pass_schedule(*args, out, 8) < 0 and _lib.last_error()


def test_no_gpu_means_the_pass_entry_points_fail_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((16, 16))
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.Plan(sc, 16, 4, pass_samples=4)
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.PathIntegrator(pa.BlueSampler(16), 4).render(sc, pass_samples=4)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = ["queue", "mega", "scene"]  # stage-queued precompiled | megakernel | the scene's own kernel (compiled at plan creation)


@pytest.fixture(scope="module")
def kernel_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("kernel_cache"))


def _kernel_env(monkeypatch, kernel, kernel_cache):
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    monkeypatch.setenv("PINE_GPU_SPECIALIZE", "1" if kernel == "scene" else "0")
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", kernel_cache)
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")


def _pass_sizes(spp):
    """k (asked for as 1: the planner rounds up), spp / 4, spp / 2, a value that does not divide spp, spp."""
    odd = next((p for p in (spp // 3 + 1, spp // 2 + 1, spp - 1) if 1 < p < spp and spp % p), None)
    return sorted({1, max(1, spp // 4), max(1, spp // 2), spp} | ({odd} if odd else set()))


def _render_passes(scene, spp, depth, P, each=None, **kw):
    """The film after the last pass of a plan with passes (each(j, film, plan) sees every intermediate film)."""
    import torch
    import pine_amd as pa
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, spp, depth, pass_samples=P, **kw)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for j in range(plan.pass_count):
            plan.launch_pass(j, film.data_ptr(), stream)
            if each is not None:
                torch.cuda.synchronize()
                plan.check()
                each(j, film.cpu().numpy(), plan)
        torch.cuda.synchronize()
        plan.check()
        return film.cpu().numpy(), plan.pass_count
    finally:
        plan.close()


def _sampler(name, spp):
    import pine_amd as pa
    return pa.SobolSampler(spp) if name.startswith("sobol_") else pa.HaltonSampler(spp) if name.startswith("halton_") else spp


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", FILM_NAMES + SOBOL_FILM_NAMES + HALTON_FILM_NAMES)
def test_final_film_of_a_render_in_passes_is_the_reference_film(name, kernel, monkeypatch, kernel_cache):
    """Every pine-order golden film of the real reference, rendered in passes of every size class: bit for bit."""
    _kernel_env(monkeypatch, kernel, kernel_cache)
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    assert sc.describe() == ps
    counts = []
    for P in _pass_sizes(spp):
        film, n = _render_passes(sc, _sampler(name, spp), depth, P)
        counts.append(n)
        assert_bit_equal(film, ref, f"{name} {kernel} pass_samples={P} ({n} passes)")
    assert max(counts) > 1 or spp == 1, counts


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", EMBREE_FILM_NAMES + EMBREE_MORE_FILM_NAMES)
def test_final_film_in_passes_in_embree_order(name, kernel, monkeypatch, kernel_cache):
    _kernel_env(monkeypatch, kernel, kernel_cache)
    ref, ps, spp, depth = load_film(name)
    sc = embree_scene(name)
    assert sc.describe() == ps
    for P in _pass_sizes(spp):
        film, n = _render_passes(sc, spp, depth, P, order="embree")
        assert_bit_equal(film, ref, f"{name} {kernel} pass_samples={P} ({n} passes)")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["queue", "mega"])
@pytest.mark.parametrize("name", FILM_NAMES + SOBOL_FILM_NAMES + HALTON_FILM_NAMES)
def test_shards_and_packed_slabs_of_a_render_in_passes(name, kernel, monkeypatch, kernel_cache):
    """World 2: the two final films summed, and the two packed slabs unpacked, equal the reference film."""
    import torch
    import pine_amd as pa
    _kernel_env(monkeypatch, kernel, kernel_cache)
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    h, w = ref.shape[:2]
    P = max(1, spp // 4)
    tot = np.zeros_like(ref)
    slabs = []
    stream = torch.cuda.current_stream().cuda_stream
    for r in range(2):
        f, _ = _render_passes(sc, _sampler(name, spp), depth, P, shard_rank=r, shard_world=2)
        tot += f
        plan = pa.Plan(sc, _sampler(name, spp), depth, pass_samples=P, shard_rank=r, shard_world=2)
        slab = torch.full((plan.slab_floats(),), -7.0, dtype=torch.float32, device="cuda")
        plan.launch_packed(slab.data_ptr(), stream)  # (all passes, in order)
        torch.cuda.synchronize()
        plan.check()
        plan.close()
        slabs.append(slab)
    assert_bit_equal(tot, ref, f"{name}: sum of 2 shards")
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    pa.film_unpack((w, h), 2, torch.stack(slabs).data_ptr(), film.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert_bit_equal(film.cpu().numpy(), ref, f"{name}: packed slabs")


@pytest.mark.gpu
@pytest.mark.parametrize("name,passes", [("C2_cbox_640_s256_d8_readme", 8), ("C5_sss_320_s512_d8", 4)])
def test_full_size_in_passes_md5(name, passes, monkeypatch):
    from pine_amd import scenes
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    st = json.load(open(os.path.join(GOLDEN, "stats_640.json")))[name]
    sc = scenes.cbox((640, 640), "readme") if name.startswith("C2") else scenes.sss((320, 320), 3)
    spp = min(256, st["spp"])  # BlueSampler(512) renders 256
    film, n = _render_passes(sc, st["spp"], st["depth"], spp // passes, specialize=False)
    assert n == passes
    assert hashlib.md5(film.tobytes()).hexdigest() == st["md5"]


def _whole_pixel_tiles(plan, spp):
    st = plan.stats()
    order = plan.tile_order()
    return order[:st.serial_tiles] if st.serial_tiles > 0 else (order if st.samples_per_item == spp else [])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["queue", "mega"])
@pytest.mark.parametrize("name", ["cbox_readme_64_s16_d4", "lights_zoo_64_s32_d6", "sss_48_s32_d8"])
def test_every_intermediate_film_is_the_partial_sum_it_claims(name, kernel, monkeypatch, kernel_cache):
    """Per-sample radiance of an ordinary plan, summed left to right in float32 on the host: the film after pass j is
    partial_sum(m) / m for pixels of the independent class (m = samples so far); a whole-pixel tile is final once its slice
    has run and (0, 0, 0, 0) before."""
    import torch
    import pine_amd as pa
    _kernel_env(monkeypatch, kernel, kernel_cache)
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    h, w = ref.shape[:2]
    plan = pa.Plan(sc, spp, depth)
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    samples = plan.read_samples()[..., :3]                                       # [h, w, spp, 3]
    plan.close()
    zero = np.zeros((h, w, 1, 3), np.float32)
    partial = np.cumsum(np.concatenate([zero, samples], axis=2), axis=2, dtype=np.float32)  # sequential: partial[m] = ((0 + L_0) + ...) + L_{m-1}
    tiles_x = (w + 7) // 8
    ys, xs = np.mgrid[0:h, 0:w]
    tile_of = (ys // 8) * tiles_x + xs // 8
    seen = []

    def each(j, got, p):
        s0, ns, t0, nt = p.pass_info(j)
        m = s0 + ns
        whole = _whole_pixel_tiles(p, spp)
        want = np.concatenate([partial[:, :, m] / np.float32(m), np.ones((h, w, 1), np.float32)], axis=2)
        done, pending = np.isin(tile_of, whole[:t0 + nt]), np.isin(tile_of, whole[t0 + nt:])
        want[done] = ref[done]
        want[pending] = 0.0
        assert_bit_equal(got, want, f"{name} {kernel}: film after pass {j} of {p.pass_count}")
        seen.append((len(whole), int(pending.sum())))

    for P in (max(1, spp // 4), 5):
        film, n = _render_passes(sc, spp, depth, P, each=each)
        assert n > 1
        assert_bit_equal(film, ref, name)
    if name.startswith("sss") and kernel == "queue":
        assert seen[0][0] > 0 and seen[0][1] > 0, "the Subsurface scene has whole-pixel tiles that wait for their slice"


@pytest.mark.gpu
def test_device_memory_is_that_of_one_pass(monkeypatch):
    import pine_amd as pa
    from pine_amd import scenes
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    for sc, size, spp, depth, P in [(scenes.cbox((64, 64), "readme"), (64, 64), 16, 4, 6), (scenes.sss((48, 48), 1), (48, 48), 32, 8, 8),
                                    (scenes.cbox((640, 640), "readme"), (640, 640), 256, 8, 32)]:
        plan = pa.Plan(sc, spp, depth, pass_samples=P, specialize=False)
        st = plan.stats()
        tiles = _local_tiles(*size, 0, 1)
        k = spp if (st.serial_tiles == 0 and st.samples_per_item == spp) else st.samples_per_item
        s = _schedule(*size, 0, 1, spp, k, st.serial_tiles, P)
        whole = tiles if k == spp else st.serial_tiles
        rows = (s[:, 3] * spp + (tiles - whole) * s[:, 1]).max()
        got = plan.device_bytes()
        assert plan.pass_count == len(s) > 1
        assert got[0] == rows * 64 * 16
        assert got[1] == ((tiles - whole) * (s[:, 1].max() // k) * 64 * 16 if k < spp else 0)
        assert got[2] == tiles * 64 * 16 + ((tiles - whole) * 64 * 16 if k < spp else 0)
        assert got[3] >= got[0] + got[1] + got[2]
        plan.close()
        if size == (640, 640):
            plain = pa.Plan(sc, spp, depth, specialize=False)
            whole_bytes = plain.device_bytes()
            plain.close()
            assert whole_bytes[2] == 0 and whole_bytes[0] == tiles * spp * 64 * 16
            assert got[0] + got[1] <= (whole_bytes[0] + whole_bytes[1]) // 8 + tiles * 64 * 16


@pytest.mark.gpu
def test_a_render_one_launch_refuses_runs_in_passes(monkeypatch):
    """3840 x 2160, SobolSampler(1024): one launch would need a 33-bit sample index; 16 samples per pass do not.  (One pass
    only: there is no reference film of that size.)"""
    import torch
    import pine_amd as pa
    from pine_amd import scenes
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    sc = scenes.cbox((3840, 2160), "readme")
    with pytest.raises(pa.PineError, match="2\\^32"):
        pa.Plan(sc, pa.SobolSampler(1024), 4, specialize=False)
    plan = pa.Plan(sc, pa.SobolSampler(1024), 4, specialize=False, pass_samples=16)
    assert plan.pass_count == 64
    film = torch.zeros((2160, 3840, 4), dtype=torch.float32, device="cuda")
    plan.launch_pass(0, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    out = film.cpu().numpy()
    assert (out[..., 3] == 1.0).all() and np.isfinite(out).all() and out[..., :3].max() > 0
    plan.close()


@pytest.mark.gpu
def test_pass_protocol(monkeypatch):
    import torch
    import pine_amd as pa
    from pine_amd import scenes, _lib
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    sc = scenes.cbox((64, 64), "readme")
    stream = torch.cuda.current_stream().cuda_stream
    film = torch.full((64, 64, 4), -3.0, dtype=torch.float32, device="cuda")
    plan = pa.Plan(sc, 16, 4, pass_samples=4, specialize=False)
    assert plan.pass_count == 4 and pa.Plan(sc, 16, 4, specialize=False).pass_count == 1
    assert pa.Plan(sc, 16, 4, pass_samples=0, specialize=False).pass_count == 1 and pa.Plan(sc, 16, 4, pass_samples=99, specialize=False).pass_count == 1
    # out of order: an error, and nothing is launched (the film keeps what it held)
    with pytest.raises(pa.PineError, match="order"):
        plan.launch_pass(2, film.data_ptr(), stream)
    torch.cuda.synchronize()
    assert (film.cpu().numpy() == -3.0).all()
    plan.launch_pass(0, film.data_ptr(), stream)
    with pytest.raises(pa.PineError, match="order"):
        plan.launch_pass(3, film.data_ptr(), stream)
    with pytest.raises(pa.PineError, match="order"):
        plan.launch_pass(4, film.data_ptr(), stream)
    plan.launch_pass(1, film.data_ptr(), stream)
    v1 = plan.stats().vertices
    with pytest.raises(pa.PineError, match="ordinary plan"):
        plan.read_samples()
    # pass 0 again starts afresh; launch() runs all passes; the statistics are those of the whole sequence
    plan.launch_pass(0, film.data_ptr(), stream)
    plan.launch(film.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = pa.PathIntegrator(pa.BlueSampler(16), 4).render(sc).pixels
    assert_bit_equal(film.cpu().numpy(), ref, "launch() of a plan with passes")
    whole = pa.Plan(sc, 16, 4, specialize=False)
    whole.launch(film.data_ptr(), stream)
    a, b = plan.stats(), whole.stats()
    assert (a.vertices, a.shadow_rays) == (b.vertices, b.shadow_rays) and 0 < v1 < a.vertices
    plan.close()
    whole.close()
    # the one-shot form: a callback that stops after pass 1 leaves the film of pass 1
    films = []

    def on_pass(j, n, f):
        films.append(f.copy())
        return j == 1

    integ = pa.PathIntegrator(pa.BlueSampler(16), 4, specialize=False)
    out = integ.render(sc, pass_samples=4, on_pass=on_pass).pixels
    assert integ.stopped and len(films) == 2
    assert_bit_equal(out, films[1], "the film a stopped render leaves")
    assert not np.array_equal(films[0], films[1])
    prm = _lib.RenderParams(16, 4, 0, 0, 1, 0, _lib.FLAG_NO_SPECIALIZE, 0)
    buf = np.zeros((64, 64, 4), np.float32)
    stop = _lib.PASS_CALLBACK(lambda user, j, n, f: 1 if j == 1 else 0)
    assert _lib.lib.pine_gpu_path_render_passes(sc._h, C.byref(prm), 4, buf.ctypes.data_as(_lib.c_f_p), stop, None) == _lib.RENDER_STOPPED == 1
    assert_bit_equal(buf, films[1], "PINE_GPU_RENDER_STOPPED")
    done = integ.render(sc, pass_samples=4).pixels  # no callback
    assert not integ.stopped
    assert_bit_equal(done, ref, "render(pass_samples=4)")


@pytest.mark.gpu
def test_one_pass_plan_reuses_its_checkpoints_on_another_stream(monkeypatch):
    """A plan of one pass computes its RNG checkpoints in the first launch (stream A) and keeps them; the second launch, on
    stream B with no host synchronisation in between, reuses the table behind the plan's checkpoint event.  (B is ordered behind
    A on the device: the plan's launch buffers serve one launch at a time.)"""
    import torch
    import pine_amd as pa
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    name = "cbox_committed_ragged_45x37_s8_d3"
    ref, ps, spp, depth = load_film(name)
    plan = pa.Plan(film_scene(name), spp, depth, specialize=False)
    assert plan.pass_count == 1
    assert plan.device_bytes()[1] > 0, "the plan uses no checkpoints: this test would check nothing"
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    films = [torch.full(ref.shape, -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()  # (the fills ran on the current stream)
    plan.launch(films[0].data_ptr(), a.cuda_stream)
    b.wait_stream(a)
    plan.launch(films[1].data_ptr(), b.cuda_stream)
    a.synchronize()
    b.synchronize()
    plan.check()
    plan.close()
    for i, film in enumerate(films):
        assert_bit_equal(film.cpu().numpy(), ref, f"{name}: film {i + 1} of two streams")


@pytest.mark.gpu
def test_a_bailed_out_pass_fails_check_and_stats(monkeypatch):
    """PINE_GPU_FLAG_DEBUG_FORCE_BAIL (the existing test hook) in pass 0 of a plan with passes: check() and stats() fail."""
    import torch
    import pine_amd as pa
    from pine_amd import scenes, _lib
    monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    sc = scenes.cbox((64, 64), "readme")
    plan = pa.Plan(sc, 8, 4, flags=_lib.FLAG_DEBUG_FORCE_BAIL, pass_samples=2, specialize=False)
    film = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")
    plan.launch_pass(0, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(pa.PineError, match="bailed out"):
        plan.check()
    with pytest.raises(pa.PineError, match="bailed out"):
        plan.stats()
    plan.close()
