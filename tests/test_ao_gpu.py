"""AOIntegrator on the GPU: every film of the real reference's AOIntegrator(BVH(), sampler) (tests/golden/ao_*.npz), bit
for bit and without a tolerance, from the regrouped kernel and from its plain twin, from both sampler tables of kernel
variants; shards, determinism, the refusals, the PRL front-end."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal
from ao_scenes import AO_FILMS, ao_sampler, ao_scene

pytestmark = pytest.mark.gpu

# kernel variants (pine_ao_kernel.h): 0 / 1 analytic shapes with the scene in LDS, BlueSampler / all samplers; 2 / 3 every shape
# kind from global memory, BlueSampler / all samplers
ANALYTIC_IN_LDS = {"cbox_readme_64_s64", "cbox_ragged_45x37_s16", "cbox_readme_24_s4", "zoo_48_s32", "sobol_cbox_32_s24",
                   "halton_zoo_32_s16", "lens_zoo_32_s16"}


def variants_of(name):
    """(variant index or None for the library's choice) the film must come out of."""
    blue = AO_FILMS[name][0] == "blue"
    out = [None]
    if name in ANALYTIC_IN_LDS:
        out += [0, 1] if blue else [1]
    out += [2, 3] if blue else [3]
    return out


def fixture(name):
    z = np.load(os.path.join(GOLDEN, f"ao_{name}.npz"))
    return z["film"], int(z["spp"])


def render_plan(name, **kw):
    import torch
    import pine_amd as pa
    scene = ao_scene(name)
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, ao_sampler(name), 1, integrator="ao", **kw)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.check()
    return plan, film.cpu().numpy()


CASES = [(n, k, v) for n in sorted(AO_FILMS) for k in ("regroup", "serial") for v in variants_of(n)]


@pytest.mark.parametrize("name,kernel,variant", CASES, ids=[f"{n}-{k}-{'auto' if v is None else v}" for n, k, v in CASES])
def test_film_is_the_reference_film(name, kernel, variant, monkeypatch):
    monkeypatch.setenv("PINE_GPU_AO_KERNEL", kernel)
    if variant is not None:
        monkeypatch.setenv("PINE_GPU_AO_VARIANT", str(variant))
    want, spp = fixture(name)
    plan, got = render_plan(name)
    st = plan.stats()
    assert st.spp_effective == spp
    assert st.shadow_rays == 8 * st.vertices and st.vertices > 0
    assert st.camera_samples == want.shape[0] * want.shape[1] * spp
    assert_bit_equal(got, want, f"{name} {kernel} variant {variant}")


def test_one_shot_render():
    import pine_amd as pa
    name = "cbox_readme_24_s4"
    film = pa.AOIntegrator(ao_sampler(name)).render(ao_scene(name)).pixels
    assert_bit_equal(film, fixture(name)[0], name)


def test_shards_sum_to_the_film():
    import pine_amd as pa
    name = "cbox_ragged_45x37_s16"
    want, _ = fixture(name)
    total = np.zeros_like(want)
    for rank in range(3):
        _, part = render_plan(name, shard_rank=rank, shard_world=3)
        for y in range(want.shape[0]):
            for x in range(want.shape[1]):
                if pa._lib.lib.pine_gpu_shard_of_pixel(want.shape[1], x, y, 3) != rank:
                    assert not part[y, x].view(np.uint32).any(), (rank, x, y)  # exact zeros outside the shard
        total += part
    assert_bit_equal(total, want, "sum of three shards")


def test_two_launches_one_film():
    import torch
    plan, first = render_plan("zoo_48_s32", timing=True)
    film = torch.zeros(first.shape, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.check()
    assert_bit_equal(film.cpu().numpy(), first, "second launch")
    st = plan.stats()
    assert st.shadow_rays == 8 * st.vertices
    assert st.trace_ms > 0 and st.grid_blocks > 0 and st.block_threads == 256 and st.lds_bytes > 0


def test_second_launch_on_another_stream_waits_for_the_checkpoints():
    """AO count 2: a pixel is two items, the second starts from an RNG checkpoint.  The first launch computes the table on
    stream A; the second, on stream B, reuses it behind the plan's checkpoint event.  No host synchronisation in between.  (B is
    ordered behind A on the device: the plan's launch buffers serve one launch at a time.)"""
    import torch
    import pine_amd as pa
    name = "cbox_ragged_45x37_s16"
    want, spp = fixture(name)
    assert spp >= 2
    plan = pa.Plan(ao_scene(name), ao_sampler(name), 1, integrator="ao")
    assert plan.device_bytes()[1] > 0
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    films = [torch.full(want.shape, -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()  # (the fills ran on the current stream)
    plan.launch(films[0].data_ptr(), a.cuda_stream)
    b.wait_stream(a)
    plan.launch(films[1].data_ptr(), b.cuda_stream)
    a.synchronize()
    b.synchronize()
    plan.check()
    for i, film in enumerate(films):
        assert_bit_equal(film.cpu().numpy(), want, f"{name}: film {i + 1} of two streams")


def test_refusals():
    import torch
    import pine_amd as pa
    scene = ao_scene("cbox_readme_24_s4")
    for flags in (pa._lib.FLAG_ORDER_EMBREE, pa._lib.FLAG_FAST):
        with pytest.raises(pa.PineError):
            pa.Plan(scene, 16, 1, integrator="ao", flags=flags)
    with pytest.raises(pa.PineError, match=r"AOIntegrator\(BVH\(\), sampler\)"):
        pa.Plan(scene, 16, 1, integrator="ao", order="embree")
    plan = pa.Plan(scene, 16, 1, integrator="ao")
    slab = torch.zeros(plan.slab_floats(), dtype=torch.float32, device="cuda")
    with pytest.raises(pa.PineError, match="packed"):
        plan.launch_packed(slab.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(pa.PineError):
        plan.read_samples()
    with pytest.raises(pa.PineError):
        pa.Plan(scene, 16, 1, integrator="ao", pass_samples=1)


def test_a_launch_that_gives_up_fails():
    """The bail-out record is the path kernels': a launch that raised it has no film to return."""
    import torch
    import pine_amd as pa
    scene = ao_scene("cbox_readme_24_s4")
    plan = pa.Plan(scene, 16, 1, integrator="ao", flags=pa._lib.FLAG_DEBUG_FORCE_BAIL)
    film = torch.zeros((24, 24, 4), dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(pa.PineError, match="bailed out"):
        plan.check()
    with pytest.raises(pa.PineError, match="bailed out"):
        pa.AOIntegrator(pa.BlueSampler(16), flags=pa._lib.FLAG_DEBUG_FORCE_BAIL).render(scene)


def test_prl_renders_the_fixture_film():
    from pine_amd import prl
    name = "cbox_readme_64_s64"
    src = '''
scene := Scene();
scene.add("floor", Diffuse([0.9, 0.9, 0.9]));
scene.add("blue", Diffuse([0.2, 0.5, 0.9]));
scene.add("red", Diffuse([0.9, 0.1, 0.05]));
scene.add("green", Diffuse([0.2, 0.9, 0.05]));
scene.add(Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], true), "floor");
scene.add(Rect([0, 2, 1], [2, 0, 0], [0, 0, 2]), "floor");
scene.add(Rect([-1, 1, 1], [0, 0, 2], [0, 2, 0], true), "red");
scene.add(Rect([1, 1, 1], [0, 0, 2], [0, 2, 0]), "green");
scene.add(Rect([0, 1, 2], [2, 0, 0], [0, 2, 0], true), "blue");
unit := AABB([0, 0, 0], [1, 1, 1]);
scene.add(Box(unit, translate([0.0, 0.0, 0.6]) * rotate_y(0.4) * scale([0.6, 0.6, 0.6])), "floor");
scene.add(Box(unit, translate([-0.6, 0.0, 1.0]) * rotate_y(-0.4) * scale([0.6, 1.3, 0.6])), "floor");
scene.add(Rect([0.0, 2.0 - 0.1, 1], [0.1, 0, 0], [0, 0, 0.1]), Emissive(600 * [1.0, 0.64, 0.185]));  # (2.0 - 0.1: the float the fixture's scene holds)
scene.set(ThinLenCamera(Film([64, 64], Uncharted2()), [0, 1, -4], [0, 1, 0], 0.25));
AOIntegrator(BVH(), BlueSampler(64)).render(scene);
'''
    # (the script builds the scene the fixture was rendered from: its dry run says so before anything is rendered)
    dry = prl.interpret(src, dry_run=True)
    lines = dry.splitlines()
    i = next(k for k, l in enumerate(lines) if l.startswith("@render AOIntegrator"))
    j = next(k for k in range(i, len(lines)) if lines[k] == "@end")
    z = np.load(os.path.join(GOLDEN, f"ao_{name}.npz"))
    shapes = lambda text: [l for l in text.splitlines() if not l.startswith("material ")]  # (materials play no part in AO)
    assert shapes("\n".join(lines[i + 1:j])) == shapes(bytes(z["pscene"]).decode())
    prl.interpret(src)
    assert_bit_equal(prl.last_film(), z["film"], "PRL AOIntegrator(BVH(), BlueSampler(64))")
