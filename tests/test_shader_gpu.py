"""GPU (-m gpu): Shader's batched path-vertex queries (include/pine_gpu.h pine_gpu_shader_*) and the wavefront loop over them
(pine_amd.WavefrontPathIntegrator) against the real reference -- the 16 floats of every radiance() invocation of
tests/golden/vertices_*.npz, the reference's small films in both traversal orders -- and, where the reference left no small
film, against PathIntegrator on the same GPU.  Every comparison is bit for bit: zero tolerance, nothing excluded.  Sample sums
are formed by the fold kernel and films by the resolve kernel, never by torch arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

import atmosphere_scenes
import envsky_scenes
import noise_scenes
import texture_scenes
from conftest import GOLDEN, assert_bit_equal, embree_scene, load_film
from film_scenes import film_sampler, film_scene

pytestmark = pytest.mark.gpu
WORD_A, WORD_B = 0xFFFFFFFF, 0x5A5A5A5A
POISON = "PINE_GPU_TEST_POISON"
VARIANT = "PINE_GPU_SHADER_VARIANT"
NULL_RAY = np.array([0, 0, 0, 0, 0, 1, 0, -1], np.float32)
RAGGED = "cbox_committed_ragged_45x37_s8_d3"


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in (POISON, VARIANT, "PINE_GPU_ACCEL_VARIANT"):
        monkeypatch.delenv(k, raising=False)


def _sampler(name, spp):
    import pine_amd as pa
    s = film_sampler(name, spp)
    return s if hasattr(s, "requested") else pa.BlueSampler(s)


def _wavefront(scene, sampler, depth, **kw):
    import pine_amd as pa
    return pa.WavefrontPathIntegrator(sampler, depth, **kw).render(scene).pixels


# ---- 1. per-vertex terms against the real reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cbox", "mats"])
def test_per_vertex_terms_equal_the_reference(name):
    """The fold's log over the wavefront loop: the 16 floats of EVERY radiance() invocation of 256 paths (8x8 film, 4 spp) equal
    `pine_ref vertices`, the vertex count per path is the reference's with zeros behind it, and the whole log equals
    pine_gpu_plan_vertex_log of a FLAG_VERTEX_LOG plan of the same scene."""
    import torch
    import pine_amd as pa
    from pine_amd import _lib, scenes
    z = np.load(os.path.join(GOLDEN, f"vertices_{name}.npz"))
    sc = scenes.cbox((8, 8), "readme") if name == "cbox" else scenes.materials_zoo((8, 8))
    assert sc.describe() == str(z["pscene"])
    spp, depth, rec = int(z["spp"]), int(z["depth"]), z["records"]
    integrator = pa.WavefrontPathIntegrator(pa.BlueSampler(spp), depth)
    film = integrator.render(sc, vertex_log=True).pixels
    log = integrator.vertex_log
    assert log.shape == (8, 8, spp, depth, 16)
    names = ["kind", "length", "nee.x", "nee.y", "nee.z", "f.x", "f.y", "f.z", "cosine", "pdf", "is_delta", "mis", "light_pdf", "Lo.x", "Lo.y", "Lo.z"]
    i = paths = 0
    for y in range(8):
        for x in range(8):
            for s in range(spp):
                k = int(rec[i])
                r = rec[i + 1:i + 1 + 16 * k].reshape(k, 16)
                i += 1 + 16 * k
                got = log[y, x, s, :k]
                bad = np.argwhere(got.view(np.uint32) != r.view(np.uint32))
                assert bad.size == 0, (f"pixel ({x},{y}) sample {s} vertex {bad[0][0]}: {names[bad[0][1]]} {got[tuple(bad[0])]!r} vs the reference's "
                                       f"{r[tuple(bad[0])]!r}")
                assert (log[y, x, s, k:].view(np.uint32) == 0).all(), f"pixel ({x},{y}) sample {s}: more vertices than the reference's {k}"
                paths += 1
    assert i == rec.size and paths == 256
    # ... and the fused kernel's own log and film
    plan = pa.Plan(sc, spp, depth, flags=_lib.FLAG_VERTEX_LOG)
    n = _lib.lib.pine_gpu_plan_vertex_log(plan._h, None, 0)
    assert n == log.size, _lib.last_error()
    fused = torch.zeros((8, 8, 4), dtype=torch.float32, device="cuda")
    plan.launch(fused.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.check()
    plan_log = np.zeros(n, np.float32)
    assert _lib.lib.pine_gpu_plan_vertex_log(plan._h, plan_log.ctypes.data_as(_lib.c_f_p), n) == n, _lib.last_error()
    plan.close()
    assert_bit_equal(log, plan_log.reshape(log.shape), "the fold's log vs pine_gpu_plan_vertex_log")
    assert_bit_equal(film, fused.cpu().numpy(), "the wavefront film vs the plan's")


# ---- 2. films against the real reference's goldens ---------------------------------------------------------------------------
PINE_ORDER_FILMS = ["cbox_readme_64_s1_d1", RAGGED, "lights_nosky_48_s16_d4", "xshapes_nolights_40_s8_d3", "mesh_glossy_48_s32_d6",
                    "sobol_cbox_ragged_45x37_s12_d3", "sobol_mats_zoo_32_s16_d6", "halton_cbox_readme_40_s8_d4", "halton_mats_zoo_32_s12_d6"]


@pytest.mark.parametrize("name", PINE_ORDER_FILMS)
def test_films_equal_the_references_in_pine_bvh_order(name):
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    assert sc.describe() == ps
    assert_bit_equal(_wavefront(sc, _sampler(name, spp), depth), ref, name)


def test_film_equals_the_references_in_embree_order():
    """The shader is order-agnostic: with Accel(order="embree") the loop renders EmbreeAccel's film."""
    import pine_amd as pa
    name = "embree_cbox_committed_64_s16_d4"
    ref, ps, spp, depth = load_film(name)
    sc = embree_scene(name)
    assert sc.describe() == ps
    assert_bit_equal(_wavefront(sc, pa.BlueSampler(spp), depth, order="embree"), ref, name)


# ---- 3. what has no small reference film: PathIntegrator on the same GPU -------------------------------------------------------
def _image_sky():
    s = envsky_scenes._open_sun((24, 20))
    s.set(envsky_scenes.image_sky("sun"))
    return s


def _atmosphere():
    s = envsky_scenes._open_sun((24, 20))
    s.set(atmosphere_scenes.light("noon", None, atmosphere_scenes.FILM_SUN_COLOR))
    return s


SAME_GPU = {"image_sky": _image_sky, "atmosphere": _atmosphere, "textured_room": lambda: texture_scenes.room((24, 20)),
            "noise_room": lambda: noise_scenes.room((24, 20))}


@pytest.mark.parametrize("name", list(SAME_GPU))
def test_films_equal_path_integrators_on_a_ragged_film(name):
    """ImageSky, Atmosphere, image-texture nodes and noise nodes at 24x20 (480 paths: a ragged last block), 4 spp, depth 4."""
    import pine_amd as pa
    sc = SAME_GPU[name]()
    want = pa.PathIntegrator(pa.BlueSampler(4), 4, specialize=False).render(sc).pixels
    got = _wavefront(sc, pa.BlueSampler(4), 4)
    assert got.shape == (20, 24, 4) and float(got[..., :3].max()) > 0
    assert_bit_equal(got, want, name)


# ---- 4. every variant that covers the Cornell box ------------------------------------------------------------------------------
def test_every_variant_that_covers_the_cornell_box_renders_its_film(monkeypatch):
    import pine_amd as pa
    from pine_amd import scenes
    ref, ps, spp, depth = load_film(RAGGED)
    sc = film_scene(RAGGED)
    with pa.Shader(sc, pa.BlueSampler(spp), depth) as sh:
        assert sh.variant == 0 and sh.kernel_features & (1 << 8) and sh.lds_bytes > 0  # (the narrow one: F_LDS_SCENE)
    with pa.Shader(scenes.materials_zoo((8, 8)), pa.BlueSampler(4), 3) as sh:
        assert sh.variant == 1 and sh.lds_bytes == 0
    covering = []
    for index in range(8):
        monkeypatch.setenv(VARIANT, str(index))
        try:
            with pa.Shader(sc, pa.BlueSampler(spp), depth) as sh:
                assert sh.variant == index
        except pa.PineError as e:
            assert "PINE_GPU_SHADER_VARIANT" in str(e)
            continue
        covering.append(index)
        assert_bit_equal(_wavefront(sc, pa.BlueSampler(spp), depth), ref, f"variant {index}")
    assert covering == [0, 1]
    monkeypatch.setenv(VARIANT, "0")  # (the narrow variant takes no Uber material, no node program)
    with pytest.raises(pa.PineError, match="PINE_GPU_SHADER_VARIANT"):
        pa.Shader(scenes.materials_zoo((8, 8)), pa.BlueSampler(4), 3)


# ---- 5. / 6. the loop on raw buffers: edges of the batch, every output word written ------------------------------------------
def _filled(shape, word, dtype):
    import torch
    if dtype == torch.uint8:
        return torch.full(shape, word & 0xFF, dtype=torch.uint8, device="cuda")
    t = torch.full(shape, word - (1 << 32) if word >= (1 << 31) else word, dtype=torch.int32, device="cuda")
    return t if dtype == torch.int32 else t.view(torch.float32)


def _raw_loop(sc, sampler, depth, order, word):
    """The wavefront loop on buffers pre-filled with `word`: -> everything a caller can download, as numpy arrays."""
    import torch
    import pine_amd as pa
    with pa.Accel(sc, order=order) as accel, pa.Shader(sc, sampler, depth) as sh:
        n = sh.film_size[0] * sh.film_size[1]
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        states, sums = _filled((n, 8), word, i32), _filled((n, 4), word, f32)
        rays, shadow, nxt = (_filled((n, 8), word, f32) for _ in range(3))
        hits, film = _filled((n, 12), word, f32), _filled((n, 4), word, f32)
        records, occluded = _filled((sh.spp, depth, n, 16), word, f32), _filled((sh.spp, depth, n), word, u8)
        logs = _filled((sh.spp, depth, n, 16), word, f32)
        kept = []
        for s in range(sh.spp):
            sh.begin(s, states, rays)
            kept.append(rays.clone())
            for level in range(depth):
                found = accel.intersect(rays, out=hits)
                sh.vertex(rays, found, states, records[s, level], shadow, nxt)
                accel.hit(shadow, out=occluded[s, level])
                kept += [shadow.clone(), nxt.clone()]
                rays, nxt = nxt, rays
            sh.fold(records[s], occluded[s], s, sums, logs[s])
            kept.append(states.clone())
        sh.resolve(sums, film)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in [film, sums, records, occluded, logs] + kept]


def test_every_output_word_is_written():
    """Records, rays, states, sums, log and film pre-filled with 0xFFFFFFFF, then with 0x5A5A5A5A: everything downloaded is
    byte-identical between the two runs (a word that differs is a word nobody wrote) -- and the film is the reference's."""
    import pine_amd as pa
    ref, ps, spp, depth = load_film(RAGGED)
    sc = film_scene(RAGGED)
    a = _raw_loop(sc, pa.BlueSampler(spp), depth, "pine", WORD_A)
    b = _raw_loop(sc, pa.BlueSampler(spp), depth, "pine", WORD_B)
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype
        bad = np.flatnonzero(x.view(np.uint8).ravel() != y.view(np.uint8).ravel())
        assert bad.size == 0, f"output {k}: {bad.size} bytes differ between the two fills, first at byte {bad[0]}"
    assert_bit_equal(a[0].reshape(ref.shape), ref, RAGGED)
    assert (a[1][:, 3] == spp).all()  # (w: the sample count)
    # a mixed scene through the all-features variant as well (delta lobes: vertices without a shadow ray)
    name = "sobol_mats_zoo_32_s16_d6"
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    a = _raw_loop(sc, pa.SobolSampler(4), depth, "pine", WORD_A)
    b = _raw_loop(sc, pa.SobolSampler(4), depth, "pine", WORD_B)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"mats zoo, output {k}"
    flags = a[2][..., 2].view(np.uint32)
    kind = a[2][..., 0].view(np.int32)
    assert ((kind == 3) & ((flags & 1) == 0)).any() and ((kind == 3) & ((flags & 1) != 0)).any() and (kind == -1).any()


@pytest.mark.parametrize("word", [WORD_A, WORD_B], ids=["A", "B"])
def test_film_on_poisoned_library_memory_equals_the_reference(monkeypatch, word):
    """Every block the library hands out filled with the word first (PINE_GPU_TEST_POISON): the shader's and the accel's scene
    records, the sampler's tables."""
    import pine_amd as pa
    from test_poisoned_memory import poison_stats
    ref, ps, spp, depth = load_film(RAGGED)
    sc = film_scene(RAGGED)
    monkeypatch.setenv(POISON, f"{word:08X}")
    before = poison_stats()
    film = _wavefront(sc, pa.BlueSampler(spp), depth)
    after = poison_stats()
    assert after[0] > before[0] and after[1] > before[1], "nothing was poisoned: the case tested nothing"
    assert_bit_equal(film, ref, RAGGED)


@pytest.fixture(scope="module")
def batch():
    """One accel and one shader on the ragged Cornell box (1665 paths, depth 3), the first level's inputs and, computed once,
    its outputs over the whole batch."""
    import torch
    import pine_amd as pa
    sc = film_scene(RAGGED)
    accel, sh = pa.Accel(sc), pa.Shader(sc, pa.BlueSampler(8), 3)
    states0, rays = sh.begin(0)
    hits = accel.intersect(rays)
    states = states0.clone()
    rec, shadow, nxt = sh.vertex(rays, hits, states)
    torch.cuda.synchronize()
    yield {"accel": accel, "shader": sh, "states0": states0, "rays": rays, "hits": hits, "states": states, "records": rec.records, "shadow": shadow,
           "next": nxt}
    sh.close()
    accel.close()


@pytest.mark.parametrize("n", [1, 257])
def test_a_slice_of_the_paths_gives_the_slice_of_the_answers(batch, n):
    """One lane, and one lane past a block: rows 0..n of the whole batch's outputs, and nothing behind the n-th row is written."""
    import torch
    sh = batch["shader"]
    states = batch["states0"].clone()
    pad = 3
    outs = [torch.full((n + pad, c), -7.25, dtype=torch.float32, device="cuda") for c in (16, 8, 8)]
    sh.vertex(batch["rays"][:n], batch["hits"].records[:n], states[:n], outs[0][:n], outs[1][:n], outs[2][:n])
    torch.cuda.synchronize()
    for got, want in zip(outs, (batch["records"], batch["shadow"], batch["next"])):
        assert np.array_equal(got[:n].cpu().numpy().view(np.uint32), want[:n].cpu().numpy().view(np.uint32))
        assert (got[n:].cpu().numpy() == -7.25).all()
    assert np.array_equal(states[:n].cpu().numpy(), batch["states"][:n].cpu().numpy())
    assert np.array_equal(states[n:].cpu().numpy(), batch["states0"][n:].cpu().numpy())
    kinds = batch["records"][:, 0].view(torch.int32).cpu().numpy()
    assert set(np.unique(kinds)) <= {0, 1, 3} and (kinds == 3).any()


def test_zero_paths_launch_nothing(batch):
    import torch
    from pine_amd import _lib
    sh, L = batch["shader"], _lib.lib
    assert L.pine_gpu_shader_vertex_device(sh._h, None, None, 0, None, None, None, None, None) == 0
    assert L.pine_gpu_shader_fold_device(sh._h, None, None, 1, 0, 0, None, None, None) == 0
    assert L.pine_gpu_shader_resolve_device(sh._h, None, 0, None, None) == 0
    empty = batch["rays"][:0]
    rec, shadow, nxt = sh.vertex(empty, batch["hits"].records[:0], batch["states0"][:0])
    assert tuple(rec.records.shape) == (0, 16) and tuple(shadow.shape) == (0, 8) and len(rec) == 0
    assert tuple(sh.resolve(torch.empty((0, 4), device="cuda")).shape) == (0, 4)


def test_finished_paths_keep_their_state_and_get_none_records(batch):
    """After max_path_length levels every path is done: one more vertex call leaves the states byte for byte as they were and
    writes "none" records and null rays."""
    import torch
    accel, sh = batch["accel"], batch["shader"]
    states, rays = batch["states0"].clone(), batch["rays"]
    for _ in range(sh.max_path_length):
        rec, shadow, nxt = sh.vertex(rays, accel.intersect(rays), states)
        rays = nxt
    torch.cuda.synchronize()
    assert (states[:, 7] == 1).all()
    before = states.cpu().numpy().copy()
    n = 257
    rec, shadow, nxt = sh.vertex(rays[:n], accel.intersect(rays[:n]), states[:n])
    torch.cuda.synchronize()
    assert np.array_equal(states.cpu().numpy(), before)
    want = np.zeros(16, np.float32)
    want[0], want[3] = np.int32(-1).view(np.float32), -1.0
    r = rec.records.cpu().numpy()
    assert np.array_equal(r.view(np.uint32), np.broadcast_to(want.view(np.uint32), r.shape))
    assert (rec.kind == -1).all() and not rec.has_shadow_ray.any() and not rec.has_next_ray.any()
    for t in (shadow, nxt):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), np.broadcast_to(NULL_RAY.view(np.uint32), (n, 8)))


def test_bad_calls_fail_with_a_message_that_names_the_cause(batch):
    """A misaligned pointer, sample = spp, levels = max_path_length + 1, a path count out of range: refused before a launch."""
    import torch
    import pine_amd as pa
    from pine_amd import _lib
    sh, L = batch["shader"], _lib.lib
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    rays, hits, states = batch["rays"], batch["hits"].records, batch["states0"].clone()
    rec, shadow, nxt = (torch.full((8, c), 3.5, dtype=torch.float32, device="cuda") for c in (16, 8, 8))
    for args in ((p(rays, 4), p(hits), 4, p(states), p(rec), p(shadow), p(nxt)), (p(rays), p(hits), 4, p(states), p(rec, 8), p(shadow), p(nxt)),
                 (p(rays), p(hits), 4, p(states, 4), p(rec), p(shadow), p(nxt))):
        assert L.pine_gpu_shader_vertex_device(sh._h, *args, None) < 0
        assert "16-byte aligned" in _lib.last_error()
    assert L.pine_gpu_shader_vertex_device(sh._h, p(rays), p(hits), -1, p(states), p(rec), p(shadow), p(nxt), None) < 0 and "number of paths" in _lib.last_error()
    assert L.pine_gpu_shader_vertex_device(sh._h, p(rays), p(hits), 1 << 31, p(states), p(rec), p(shadow), p(nxt), None) < 0
    assert L.pine_gpu_shader_begin_device(sh._h, sh.spp, p(states), p(rays), None) < 0 and f"spp = {sh.spp}" in _lib.last_error()
    assert L.pine_gpu_shader_begin_device(sh._h, -1, p(states), p(rays), None) < 0
    records, occ, sums = torch.zeros((4, 8, 16), device="cuda"), torch.zeros((4, 8), dtype=torch.uint8, device="cuda"), torch.zeros((8, 4), device="cuda")
    assert L.pine_gpu_shader_fold_device(sh._h, p(records), p(occ), sh.max_path_length + 1, 8, 0, p(sums), None, None) < 0
    assert f"max_path_length = {sh.max_path_length}" in _lib.last_error()
    assert L.pine_gpu_shader_fold_device(sh._h, p(records), p(occ), 0, 8, 0, p(sums), None, None) < 0
    assert L.pine_gpu_shader_fold_device(sh._h, p(records), p(occ), 1, 8, sh.spp, p(sums), None, None) < 0 and "sample index" in _lib.last_error()
    assert L.pine_gpu_shader_fold_device(sh._h, p(records), p(occ), 1, 8, 0, p(sums), p(records, 4), None) < 0 and "16-byte aligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 3.5).all() for t in (rec, shadow, nxt)) and np.array_equal(states.cpu().numpy(), batch["states0"].cpu().numpy())
    # the refusals of creation, on a machine that has a GPU
    sc = film_scene(RAGGED)
    with pytest.raises(pa.PineError, match="FLAG_ORDER_EMBREE"):
        pa.Shader(sc, pa.BlueSampler(8), 3, flags=_lib.FLAG_ORDER_EMBREE)
    with pytest.raises(pa.PineError, match="Subsurface material `skin`"):
        pa.Shader(film_scene("sss_48_s32_d8"), pa.BlueSampler(8), 3)
    for bad in (rays.double(), rays[:, :7], rays.cpu()):
        with pytest.raises(ValueError):
            sh.vertex(bad, hits, states)
    with pytest.raises(ValueError, match="written over"):
        sh.vertex(rays, hits, states, next_rays=rays)
    # a scene without a camera: creation succeeds, begin refuses
    s = pa.Scene()
    s.add(pa.Sphere([0, 0, 0], 1.0), pa.Diffuse([0.5, 0.5, 0.5]))
    with pa.Shader(s, pa.BlueSampler(4), 3) as nocam:
        assert nocam.film_size == (0, 0)
        assert L.pine_gpu_shader_begin_device(nocam._h, 0, p(states), p(rays), None) < 0 and "no camera" in _lib.last_error()


def test_the_loop_on_another_stream_gives_the_same_film():
    import torch
    import pine_amd as pa
    ref, ps, spp, depth = load_film(RAGGED)
    sc = film_scene(RAGGED)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        film = _wavefront(sc, pa.BlueSampler(spp), depth)
    stream.synchronize()
    assert_bit_equal(film, ref, RAGGED)


def test_closed_shaders_leave_nothing_behind():
    """pine_gpu_test_live_device_blocks is back where it was after a shader was made, used and closed, and after one whose
    creation failed behind the upload."""
    import gc
    import torch
    import pine_amd as pa
    from pine_amd import _lib, scenes

    def live():
        out = (C.c_int64 * 2)()
        _lib.check(_lib.lib.pine_gpu_test_live_device_blocks(out))
        return int(out[0])

    gc.collect()
    torch.cuda.synchronize()
    start = live()
    sh = pa.Shader(film_scene(RAGGED), pa.BlueSampler(8), 3)
    assert live() > start
    sh.begin(0)
    sh.close()
    sh.close()
    with pytest.raises(pa.PineError, match="closed"):
        sh.begin(0)
    assert live() == start
    os.environ[VARIANT] = "0"
    try:
        with pytest.raises(pa.PineError, match="PINE_GPU_SHADER_VARIANT"):
            pa.Shader(scenes.materials_zoo((8, 8)), pa.BlueSampler(4), 3)
    finally:
        del os.environ[VARIANT]
    assert live() == start


def test_the_wavefront_example_writes_two_pictures(tmp_path):
    """examples/wavefront_path.py at 32 x 32: the film is PathIntegrator's, the albedo AOV is the box's wall colours."""
    import importlib.util
    import pine_amd as pa
    from pine_amd import scenes
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("wavefront_path", os.path.join(ROOT, "examples", "wavefront_path.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    film, albedo = mod.render(32, 4, 3)
    want = pa.PathIntegrator(pa.BlueSampler(4), 3, specialize=False).render(scenes.cbox((32, 32), "readme")).pixels
    assert_bit_equal(film, want, "the example's film")
    assert albedo.shape == (32, 32, 4) and np.isfinite(albedo).all() and 0 <= albedo.min() and albedo.max() <= 1
    assert len(np.unique(albedo[..., :3].reshape(-1, 3).round(3), axis=0)) >= 3, "a flat albedo picture"
    mod.main(["wavefront_path.py", "16", "2", str(tmp_path / "a.png"), str(tmp_path / "b.png")])
    assert os.path.getsize(tmp_path / "a.png") > 0 and os.path.getsize(tmp_path / "b.png") > 0
