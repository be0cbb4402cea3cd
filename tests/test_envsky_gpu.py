"""ImageSky on the device: the per-call functions and whole films against fixtures made by the real reference
(tools/make_golden_envsky.py), bit for bit -- both path kernels, the scene's own kernel (baked and not), sample passes, the
Embree traversal order."""
import os

import numpy as np
import pytest

import envsky_scenes as E
from test_envsky import GOLDEN, _lib, env_records, first_difference, pa, sky_scene

pytestmark = pytest.mark.gpu


def golden_film(name):
    return np.load(os.path.join(GOLDEN, f"envsky_film_{name}.npz"))["film"]


def render(name, **kw):
    depth = E.FILMS[name][4]
    passes = kw.pop("pass_samples", None)
    integ = pa.PathIntegrator(E.film_sampler(name), depth, device=0, **kw)
    return integ.render(E.film_scene(name), pass_samples=passes).pixels


def assert_film(got, name, what):
    want = golden_film(name)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{name} ({what}): {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("name", list(E.IMAGES))
def test_device_records_equal_the_references(name):
    fx = np.load(os.path.join(GOLDEN, f"envsky_{name}.npz"))
    got = env_records(sky_scene(name), fx["queries"], 0)
    assert first_difference(got, fx["records"]) is None


@pytest.mark.parametrize("kernel", ["queue", "mega"])
@pytest.mark.parametrize("name", list(E.FILMS))
def test_films_equal_the_references(name, kernel, monkeypatch):
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    else:
        monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    assert_film(render(name, specialize=False), name, kernel)


@pytest.mark.parametrize("bake", [True, False])
def test_open_sun_with_the_scenes_own_kernel(bake, monkeypatch, tmp_path):
    import torch
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
    name = "open_sun_48x32_s16_d4"
    (w, h), depth = E.FILMS[name][1], E.FILMS[name][4]
    # (plan creation waits for the compiler: the launch below runs the scene's own kernel)
    plan = pa.Plan(E.film_scene(name), E.film_sampler(name), depth, specialize=True, flags=0 if bake else _lib.FLAG_SPECIALIZE_NO_BAKE)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    plan.close()
    assert st.specialized == (2 if bake else 1)  # (2: feature set + baked scene)
    assert_film(film.cpu().numpy(), name, "baked" if bake else "not baked")


def test_open_sun_in_four_passes():
    name = "open_sun_48x32_s16_d4"
    assert_film(render(name, specialize=False, pass_samples=4), name, "4 passes")


def test_open_sun_in_embree_order():
    """No shape of this scene depends on the traversal order, so EmbreeAccel's order renders the same film."""
    name = "open_sun_48x32_s16_d4"
    assert_film(render(name, specialize=False, order="embree"), name, "embree order")


def test_prl_script_renders_the_const_film():
    """examples/image_sky.pine with the accel named (a script's two-argument PathIntegrator takes the reference's default accel,
    EmbreeAccel; the fixtures are PathIntegrator(BVH(), ...))."""
    from pine_amd import prl
    root = os.path.dirname(os.path.dirname(GOLDEN))
    src = open(os.path.join(root, "examples", "image_sky.pine")).read().replace('world.camera.film().save("image_sky.png");', "")
    named = src.replace("PathIntegrator(BlueSampler(8), 3)", "PathIntegrator(BVH(), BlueSampler(8), UniformLightSampler(), 3)")
    assert named != src
    prl.interpret(named)
    assert_film(np.ascontiguousarray(prl.last_film(), dtype=np.float32), "const_24_s8_d3", "PRL script")
