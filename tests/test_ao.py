"""AOIntegrator, the parts that need no GPU: the host-side constants against the real reference's (tests/golden/ao_*.npz,
written by tools/make_golden_ao.py), the sample-count rule, the PRL front-end, the loud failure without a device and the
C++ facade example."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, assert_bit_equal
from ao_scenes import AO_FILMS, ao_sampler, ao_scene


def test_fixture_list_is_complete():
    listing = json.load(open(os.path.join(GOLDEN, "ao_films.json")))
    assert sorted(listing) == sorted(AO_FILMS)
    for name, (kind, spp) in AO_FILMS.items():
        assert (listing[name]["sampler"], listing[name]["sampler_spp"]) == (kind, spp)
        assert os.path.getsize(os.path.join(GOLDEN, f"ao_{name}.npz")) < 100 * 1024


@pytest.mark.parametrize("name", sorted(AO_FILMS))
def test_constants_equal_the_reference(name):
    """radius = min_value(scene.get_aabb().diagonal()) / 2 and directions[8], bit for bit, from the host alone."""
    import pine_amd as pa
    z = np.load(os.path.join(GOLDEN, f"ao_{name}.npz"))
    scene = ao_scene(name)
    assert scene.describe() == bytes(z["pscene"]).decode()  # (the fixture was rendered from this very scene)
    radius, directions = pa.api.ao_constants(scene)
    assert_bit_equal(np.concatenate([[radius], directions.ravel()]), z["constants"], name)
    assert pa.AOIntegrator(ao_sampler(name)).spp == int(z["spp"])


def test_effective_spp_rule():
    """max(sampler.spp() / 8, 1): BlueSampler's own count is rounded up to a power of two and clamped to 256."""
    import pine_amd as pa
    for sampler, want in [(pa.BlueSampler(4), 1), (pa.BlueSampler(16), 2), (pa.BlueSampler(300), 32),
                          (pa.SobolSampler(24), 3), (pa.SobolSampler(7), 1)]:
        assert pa.AOIntegrator(sampler).spp == want


def test_prl_dry_run():
    from pine_amd import prl
    out = prl.interpret(open(os.path.join(ROOT, "examples", "ambient_occlusion.pine")).read(), dry_run=True)
    assert "@render AOIntegrator BlueSampler 64\n" in out and "@save ambient_occlusion.png 128x128" in out
    line = ('s := Scene(); s.add(Sphere([0, 0, 2], 0.5), Diffuse([0.5, 0.5, 0.5])); s.set(ThinLenCamera(Film([8, 8]), [0, 0, 0], [0, 0, 1], 0.5)); '
            'AOIntegrator(BVH(), SobolSampler(24)).render(s);')
    assert "@render AOIntegrator SobolSampler 24\n" in prl.interpret(line, dry_run=True)


@pytest.mark.parametrize("ctor", ["AOIntegrator(BlueSampler(16))", "AOIntegrator(Embree(), BlueSampler(16))"])
def test_prl_refuses_embree_accel(ctor):
    """EmbreeAccel's hit8 is Embree's packet traversal, which nothing restates: the error names the form that renders."""
    from pine_amd import prl
    with pytest.raises(prl.PrlError, match=r"AOIntegrator\(BVH\(\), sampler\)"):
        prl.interpret(ctor + ";", dry_run=True)


def test_python_refuses_embree_order():
    import pine_amd as pa
    with pytest.raises(pa.PineError, match=r"AOIntegrator\(BVH\(\), sampler\)"):
        pa.AOIntegrator(pa.BlueSampler(16), order="embree")


def test_no_gpu_means_loud_failure():
    """No CPU path behind AOIntegrator either: without a device, rendering raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((16, 16))
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.AOIntegrator(pa.BlueSampler(16)).render(sc)
    with pytest.raises(pa.PineError):
        pa.Plan(sc, 16, 1, integrator="ao")


def test_cpp_facade_example_compiles(tmp_path):
    lib_dir = os.path.join(ROOT, "pine_amd", "lib")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "examples", "ambient_occlusion.cpp"), "-L" + lib_dir, "-lpine_gpu",
                        "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "ao_cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
