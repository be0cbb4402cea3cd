"""The denoising filter on the GPU: the gfx950 kernels of pine_amd/csrc/pine_denoise.hip write the bytes of the host-thread build
of the same functions (tests/test_denoise.py pins that build) -- on the four fixtures and on the small and ragged films, for 1,
5 and 8 iterations; in place on device memory; through PathIntegrator.render(denoise=True), Plan.denoise and the C++ example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_scenes as S
from conftest import ROOT, assert_bit_equal
from test_denoise import SMALL_FILMS, random_case

pytestmark = pytest.mark.gpu

ITERATIONS = [1, 5, 8]


def both(film, albedo, normal, **params):
    import pine_amd as pa
    return pa.denoise(film, albedo, normal, device=0, **params), pa.denoise(film, albedo, normal, device=-1, **params)


@pytest.mark.parametrize("name", list(S.DENOISE_FILMS))
def test_device_equals_host_build_on_the_fixtures(name):
    f = S.load(name)
    for iterations in ITERATIONS:
        dev, host = both(f["noisy"], f["albedo"], f["normal"], iterations=iterations)
        assert_bit_equal(dev, host, f"{name}, {iterations} iterations")
    assert not np.array_equal(host, f["noisy"])


@pytest.mark.parametrize("size", SMALL_FILMS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_build_on_small_films(size):
    film, albedo, normal = random_case(size[0], size[1], 7 + size[0], misses=size != (1, 1))
    for iterations in [0] + ITERATIONS:
        dev, host = both(film, albedo, normal, iterations=iterations)
        assert_bit_equal(dev, host, f"{size}, {iterations} iterations")


def test_other_parameters_too():
    film, albedo, normal = random_case(70, 9, 3)  # (wider than one 64-pixel row segment)
    dev, host = both(film, albedo, normal, iterations=3, normal_power_log2=2, sigma_color=0.7, sigma_albedo=0.2, eps_albedo=0.05)
    assert_bit_equal(dev, host, "70x9, other parameters")
    assert not np.array_equal(host, film)


@pytest.mark.parametrize("iterations", [0, 1, 2, 5])
def test_device_entry_point_in_place_and_out_of_place(iterations):
    import torch
    import pine_amd as pa
    from pine_amd import _lib
    f = S.load("xshapes_48")
    h, w = f["noisy"].shape[:2]
    want = pa.denoise(f["noisy"], f["albedo"], f["normal"], device=-1, iterations=iterations)
    prm = pa.api.denoise_params(iterations=iterations, device=0)
    film = torch.from_numpy(f["noisy"]).cuda()
    albedo = torch.from_numpy(f["albedo"]).cuda()
    normal = torch.from_numpy(f["normal"]).cuda()
    out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.lib.pine_gpu_denoise_device(C.byref(prm), w, h, ptr(film), ptr(albedo), ptr(normal), ptr(out), stream), "denoise")
    assert_bit_equal(out.cpu().numpy(), want, "out != film")
    assert_bit_equal(film.cpu().numpy(), f["noisy"], "the film is left alone")
    _lib.check(_lib.lib.pine_gpu_denoise_device(C.byref(prm), w, h, ptr(film), ptr(albedo), ptr(normal), ptr(film), stream), "denoise")
    assert_bit_equal(film.cpu().numpy(), want, "out == film")


def test_device_entry_point_refuses_the_host_build():
    import pine_amd as pa
    from pine_amd import _lib
    prm = pa.api.denoise_params(device=-1)
    one = C.c_void_p(16)
    assert _lib.lib.pine_gpu_denoise_device(C.byref(prm), 4, 4, one, one, one, one, None) < 0
    assert "device >= 0" in _lib.last_error()


def test_path_integrator_denoise_is_render_guides_denoise():
    import pine_amd as pa
    scene = S.denoise_scene("cbox_ragged_45x37")
    integ = pa.PathIntegrator(pa.BlueSampler(8), 3, specialize=False)
    plain = integ.render(scene).pixels.copy()
    albedo, normal = pa.guides(scene)
    want = pa.denoise(plain, albedo, normal)
    got = integ.render(scene, denoise=True).pixels
    assert_bit_equal(got, want, "render(denoise=True)")
    assert not np.array_equal(got, plain)
    # ... and DenoiseIntegrator on the film the camera holds, with parameters
    scene.camera.film().pixels = plain.copy()
    got = pa.DenoiseIntegrator(iterations=2, sigma_color=0.5).render(scene).pixels
    assert_bit_equal(got, pa.denoise(plain, albedo, normal, iterations=2, sigma_color=0.5), "DenoiseIntegrator(iterations=2, sigma_color=0.5)")


def test_plan_denoise_stays_on_the_device():
    import torch
    import pine_amd as pa
    scene = S.denoise_scene("cbox_ragged_45x37")
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, 8, 3, specialize=False)
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.check()
    plain = film.cpu().numpy()
    albedo, normal = pa.guides(scene)
    assert plan.denoise(film) is film
    assert_bit_equal(film.cpu().numpy(), pa.denoise(plain, albedo, normal, device=-1), "Plan.denoise")
    plan.close()


def png_pixels(path):
    """The (H, W, 4) uint8 pixels of an 8-bit RGBA PNG whose rows are unfiltered (what png_writer.hpp writes)."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 6)
            size = (h, w)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], size[1] * 4 + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(size[0], size[1], 4)


def test_cpp_example_writes_a_png(tmp_path):
    """examples/denoise.cpp, built by build(): renders, denoises through pine::DenoiseIntegrator and saves PNGs; the denoised one
    is the film of the same steps through the Python layer."""
    import pine_amd as pa
    from pine_amd import scenes
    exe = os.path.join(ROOT, "build", "denoise_cpp")
    assert os.access(exe, os.X_OK), "build/denoise_cpp missing: build() compiles examples/denoise.cpp"
    out = tmp_path / "cbox"
    r = subprocess.run([exe, os.path.join(ROOT, "pine_amd", "data", "bluesobol_u8.bin"), "40", "8", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scene = scenes.cbox((40, 40), "readme")
    film = pa.PathIntegrator(pa.BlueSampler(8), 5).render(scene)
    noisy_u8 = film.finalize_u8()
    film = pa.DenoiseIntegrator(sigma_color=0.25).render(scene)
    want_u8 = film.finalize_u8()
    for suffix, want in (("_noisy.png", noisy_u8), ("_denoised.png", want_u8)):
        got = png_pixels(str(out) + suffix)
        assert got.shape == want.shape and np.array_equal(got, want), suffix
    assert not np.array_equal(noisy_u8, want_u8)


CLI_SCRIPT = '''
scene := Scene();
scene.add("white", Diffuse([0.75, 0.75, 0.75]));
scene.add("red", Diffuse([0.875, 0.125, 0.0625]));
scene.add(Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], true), "white");
scene.add(Rect([0, 1, 2], [2, 0, 0], [0, 2, 0], true), "red");
scene.add(Sphere([0.0, 0.375, 1.0], 0.375), "white");
scene.add(Rect([0.0, 1.875, 1], [0.5, 0, 0], [0, 0, 0.5]), Emissive([20.0, 18.0, 15.0]));
scene.set(ThinLenCamera(Film([40, 24], Uncharted2()), [0, 1, -4], [0, 1, 0], 0.25));
PathIntegrator(BVH(), BlueSampler(8), UniformLightSampler(), 4).render(scene);
scene.camera.film().save("%s");
'''


def test_command_line_denoise_and_guides(tmp_path):
    """pine-mi355x --denoise filters before the script's save; --guides PREFIX writes the two guide images."""
    import pine_amd as pa
    exe = os.path.join(ROOT, "build", "pine-mi355x")
    assert os.access(exe, os.X_OK)
    script = tmp_path / "s.pine"
    plain_png, den_png = tmp_path / "plain.png", tmp_path / "den.png"
    for png, extra in ((plain_png, []), (den_png, ["--denoise", "--guides", str(tmp_path / "g")])):
        script.write_text(CLI_SCRIPT % png)
        r = subprocess.run([exe, "--tables", os.path.join(ROOT, "pine_amd", "data", "bluesobol_u8.bin")] + extra + [str(script)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    scene = pa.Scene()
    scene.add("white", pa.Diffuse([0.75, 0.75, 0.75]))
    scene.add("red", pa.Diffuse([0.875, 0.125, 0.0625]))
    scene.add(pa.Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], True), "white")
    scene.add(pa.Rect([0, 1, 2], [2, 0, 0], [0, 2, 0], True), "red")
    scene.add(pa.Sphere([0.0, 0.375, 1.0], 0.375), "white")
    scene.add(pa.Rect([0.0, 1.875, 1], [0.5, 0, 0], [0, 0, 0.5]), pa.Emissive([20.0, 18.0, 15.0]))
    scene.set(pa.ThinLenCamera(pa.Film([40, 24], pa.Uncharted2()), [0, 1, -4], [0, 1, 0], 0.25))
    # (the script builds this scene: its dry run says so -- every literal is a dyadic number, PRL and Python read them alike)
    from pine_amd import prl
    dry = prl.interpret(CLI_SCRIPT % "x.png", dry_run=True).splitlines()
    i = next(k for k, l in enumerate(dry) if l.startswith("@render PathIntegrator"))
    j = next(k for k in range(i, len(dry)) if dry[k] == "@end")
    assert dry[i + 1:j] == scene.describe().splitlines()
    film = pa.PathIntegrator(pa.BlueSampler(8), 4).render(scene)
    assert np.array_equal(png_pixels(str(plain_png)), film.finalize_u8())
    albedo, normal = pa.guides(scene)
    film = pa.DenoiseIntegrator().render(scene)
    assert np.array_equal(png_pixels(str(den_png)), film.finalize_u8())
    assert not np.array_equal(png_pixels(str(den_png)), png_pixels(str(plain_png)))
    to_u8 = lambda img: (np.clip(img[::-1], 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)  # noqa: E731
    got = png_pixels(str(tmp_path / "g_albedo.png"))
    assert np.array_equal(got[..., :3], to_u8(albedo)) and (got[..., 3] == 255).all()
    got = png_pixels(str(tmp_path / "g_normal.png"))
    assert np.array_equal(got[..., :3], to_u8(normal * np.float32(0.5) + np.float32(0.5)))
    assert (~S.hits(normal)).any() and S.hits(normal).any()


def test_nothing_is_left_behind():
    """Every device handle the new entry points take goes back (pine_gpu_test_live_device_blocks)."""
    import gc
    import pine_amd as pa
    from pine_amd import _lib
    out = (C.c_int64 * 2)()

    def live():
        _lib.check(_lib.lib.pine_gpu_test_live_device_blocks(out), "live")
        return int(out[0])
    scene = S.denoise_scene("cbox_ragged_45x37")
    f = S.load("xshapes_48")
    gc.collect()
    before = live()
    pa.guides(scene)
    pa.denoise(f["noisy"], f["albedo"], f["normal"])
    with pytest.raises(pa.PineError):
        pa.guides(scene, order="embree")
    with pytest.raises(pa.PineError):
        pa.denoise(f["noisy"], f["albedo"], f["normal"], iterations=9)
    gc.collect()
    assert live() == before
