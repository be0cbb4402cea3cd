"""Atmosphere on the device: the glibc-exact expf on every float, atmosphere_color, the table kernel against the host build,
the per-call functions and whole films against fixtures made by the real reference (tools/make_golden_atmosphere.py), bit for
bit -- both path kernels, the scene's own kernel, sample passes, the PRL script."""
import hashlib
import os

import numpy as np
import pytest

import atmosphere_scenes as A
from test_atmosphere import (GOLDEN, LISTING, _lib, atmosphere_colors, check_reference_conventions, env_table, exp_sweep, pa, prl_example, sky_scene,
                             two_light_scene)
from test_device_math import ALL
from test_envsky import env_records, env_tree, first_difference

pytestmark = pytest.mark.gpu


def golden_film(name):
    return np.load(os.path.join(GOLDEN, f"atmos_film_{name}.npz"))["film"]


def render(name, **kw):
    depth = A.FILMS[name][3]
    passes = kw.pop("pass_samples", None)
    integ = pa.PathIntegrator(A.film_sampler(name), depth, device=0, **kw)
    return integ.render(A.film_scene(name, device=0), pass_samples=passes).pixels


def assert_film(got, name, what):
    want = golden_film(name)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{name} ({what}): {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"


def test_device_expf_on_every_float():
    checked, bad = exp_sweep(0)
    assert bad is None and checked == ALL, bad


def test_device_colors_equal_the_references():
    fx = np.load(os.path.join(GOLDEN, "atmos_color.npz"))
    assert first_difference(atmosphere_colors(fx["queries"], 0), fx["colors"]) is None


@pytest.mark.parametrize("name", ["noon", "zenith", "default"])
def test_device_tables_equal_the_host_build(name):
    """atmosphere_table_kernel against the same function on host threads: the same bytes (64 x 32, the odd 33 x 17 whose grid is
    no multiple of the block, and the reference's 1024 x 1024), and the density the reference's."""
    (dd, dc), (hd, hc) = env_table(sky_scene(name, 0)), env_table(sky_scene(name))
    assert hashlib.md5(dd.tobytes()).hexdigest() == hashlib.md5(hd.tobytes()).hexdigest() == LISTING["configs"][name]["density_md5"]
    assert hashlib.md5(dc.tobytes()).hexdigest() == hashlib.md5(hc.tobytes()).hexdigest()
    assert sky_scene(name, 0).describe() == sky_scene(name).describe()


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_device_records_equal_the_references(name):
    """A device-built light: its tree is the reference's, and the device's sample / color / pdf return the reference's records."""
    fx = np.load(os.path.join(GOLDEN, f"atmos_{name}.npz"))
    scene = sky_scene(name, 0)
    tree = env_tree(scene)
    assert hashlib.md5(tree.tobytes()).hexdigest() == LISTING["configs"][name]["tree_md5"]
    assert first_difference(env_records(scene, fx["queries"], 0), fx["records"]) is None


def test_device_light_sample_distance_is_float_max():
    """The device's light_sample_other for a device-built Atmosphere: distance = float_max bit for bit, pdf not divided by the
    light count, wo and le the reference's."""
    check_reference_conventions(two_light_scene(0), 0)


@pytest.mark.parametrize("kernel", ["queue", "mega"])
@pytest.mark.parametrize("name", list(A.FILMS))
def test_films_equal_the_references(name, kernel, monkeypatch):
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    else:
        monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    assert_film(render(name, specialize=False), name, kernel)


@pytest.mark.parametrize("bake", [True, False])
def test_noon_with_the_scenes_own_kernel(bake, monkeypatch, tmp_path):
    import torch
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
    name = "noon_blue_s16_d5"
    (w, h), depth = A.FILM_SIZE, A.FILMS[name][3]
    # (plan creation waits for the compiler: the launch below runs the scene's own kernel)
    plan = pa.Plan(A.film_scene(name, device=0), A.film_sampler(name), depth, specialize=True, flags=0 if bake else _lib.FLAG_SPECIALIZE_NO_BAKE)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    plan.close()
    assert st.specialized == (2 if bake else 1)  # (2: feature set + baked scene)
    assert_film(film.cpu().numpy(), name, "baked" if bake else "not baked")


def test_low_in_four_passes():
    name = "low_blue_s16_d5"
    assert_film(render(name, specialize=False, pass_samples=4), name, "4 passes")


def test_noon_in_embree_order():
    """No shape of this scene depends on the traversal order, so EmbreeAccel's order renders the same film."""
    name = "noon_sobol_s8_d5"
    assert_film(render(name, specialize=False, order="embree"), name, "embree order")


def test_prl_script_renders_the_default_film():
    """examples/atmosphere.pine (its 0.9 spelt exactly, test_atmosphere.prl_example) with the accel named (a script's
    two-argument PathIntegrator takes the reference's default accel, EmbreeAccel; the fixtures are PathIntegrator(BVH(), ...)):
    the script's Atmosphere is the reference's 1024 x 1024 one, its tables computed on the render device."""
    from pine_amd import prl
    src = prl_example()[1].replace('world.camera.film().save("atmosphere.png");', "")
    named = src.replace("PathIntegrator(BlueSampler(16), 5)", "PathIntegrator(BVH(), BlueSampler(16), UniformLightSampler(), 5)")
    assert named != src
    prl.interpret(named)
    assert_film(np.ascontiguousarray(prl.last_film(), dtype=np.float32), "default_blue_s16_d5", "PRL script")
