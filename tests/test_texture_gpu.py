"""Image texture nodes on the device: material_params and whole films against fixtures made by the real reference
(tools/make_golden_texture.py), bit for bit -- both path kernels, the scene's own kernel (baked and not), sample passes, the
guide images."""
import os

import numpy as np
import pytest

import texture_scenes as X
from test_texture import GOLDEN, _lib, check_records, pa, zoo, zoo_fixture  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOM = "tex_room_48x32_s8_d4"


def golden_film(name):
    return np.load(os.path.join(GOLDEN, f"texture_film_{name}.npz"))["film"]


def render(name, **kw):
    size, spp, depth = X.FILMS[name]
    passes = kw.pop("pass_samples", None)
    integ = pa.PathIntegrator(pa.BlueSampler(spp), depth, device=0, **kw)
    return integ.render(X.film_scene(name), pass_samples=passes).pixels


def assert_film(got, name, what):
    want = golden_film(name)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{name} ({what}): {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"


def test_device_records_equal_the_references(zoo, zoo_fixture):  # noqa: F811
    check_records(0, zoo, zoo_fixture)


def test_the_fixture_is_the_scene_the_test_renders():
    want = bytes(np.load(os.path.join(GOLDEN, f"texture_film_{ROOM}.npz"))["pscene"]).decode()
    assert X.room(X.FILMS[ROOM][0]).describe() == want


@pytest.mark.parametrize("kernel", ["queue", "mega"])
def test_room_film_equals_the_references(kernel, monkeypatch):
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    else:
        monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    assert_film(render(ROOM, specialize=False), ROOM, kernel)


@pytest.mark.parametrize("bake", [True, False])
def test_room_with_the_scenes_own_kernel(bake, monkeypatch, tmp_path):
    import torch
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
    (w, h), spp, depth = X.FILMS[ROOM]
    # (plan creation waits for the compiler: the launch below runs the scene's own kernel)
    plan = pa.Plan(X.room((w, h)), pa.BlueSampler(spp), depth, specialize=True, flags=0 if bake else _lib.FLAG_SPECIALIZE_NO_BAKE)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    plan.close()
    assert st.specialized == (2 if bake else 1)  # (2: feature set + baked scene)
    assert_film(film.cpu().numpy(), ROOM, "baked" if bake else "not baked")


def test_room_in_four_passes():
    assert_film(render(ROOM, specialize=False, pass_samples=2), ROOM, "4 passes")


def test_room_fast_build_is_refused_like_every_node_scene():
    """PINE_GPU_FLAG_FAST covers the BASELINE scenes' feature sets, none of which has node programs (pine_kernels_fast.hip): a
    textured scene is refused by name like any other scene with node-driven materials, never rendered by another kernel."""
    size, spp, depth = X.FILMS[ROOM]
    with pytest.raises(pa.PineError, match="PINE_GPU_FLAG_FAST: no declared-tolerance kernel variant covers this scene"):
        pa.PathIntegrator(pa.BlueSampler(spp), depth, device=0, specialize=False, flags=_lib.FLAG_FAST).render(X.room(size))


@pytest.mark.parametrize("kernel", ["queue", "mega"])
def test_glb_film_equals_the_references(kernel, monkeypatch):
    """tests/golden/textured_quad.glb, loaded by the reference's own importer there and by pine_amd/gltf.py here."""
    from pine_amd import gltf
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    else:
        monkeypatch.delenv("PINE_GPU_KERNEL", raising=False)
    name, (size, spp, depth) = next(iter(X.GLB_FILMS.items()))
    scene = X.glb_scene(gltf, os.path.join(GOLDEN, "textured_quad.glb"), size)
    assert scene.describe() == bytes(np.load(os.path.join(GOLDEN, f"texture_film_{name}.npz"))["pscene"]).decode()
    film = pa.PathIntegrator(pa.BlueSampler(spp), depth, device=0, specialize=False).render(scene).pixels
    assert_film(film, name, kernel)


def test_script_room_film_equals_the_references():
    name = "tex_script_room_48x32_s8_d4"
    assert X.film_scene(name).describe() == bytes(np.load(os.path.join(GOLDEN, f"texture_film_{name}.npz"))["pscene"]).decode()
    assert_film(render(name, specialize=False), name, "queue")


def test_prl_script_renders_the_script_rooms_film():
    """examples/textured.pine with the accel named (a script's two-argument PathIntegrator takes the reference's default accel,
    EmbreeAccel; the fixtures are PathIntegrator(BVH(), ...)).  A script has no Mesh constructor, so its room is the room
    without the quad, with a reference film of its own."""
    from pine_amd import prl
    root = os.path.dirname(os.path.dirname(GOLDEN))
    src = open(os.path.join(root, "examples", "textured.pine")).read().replace("tests/golden/", GOLDEN + "/")
    src = src.replace('world.camera.film().save("textured.png");', "")
    named = src.replace("PathIntegrator(BlueSampler(8), 4)", "PathIntegrator(BVH(), BlueSampler(8), UniformLightSampler(), 4)")
    assert named != src
    prl.interpret(named)
    assert_film(np.ascontiguousarray(prl.last_film(), dtype=np.float32), "tex_script_room_48x32_s8_d4", "PRL script")


def test_room_guides_equal_the_references():
    fx = np.load(os.path.join(GOLDEN, "texture_guides_room.npz"))
    scene = X.room(X.GUIDES_SIZE)
    assert scene.describe() == bytes(fx["pscene"]).decode()
    albedo, normal = pa.guides(scene)
    for got, want, what in ((albedo, fx["albedo"], "albedo"), (normal, fx["normal"], "normal")):
        bad = (np.ascontiguousarray(got, np.float32).view(np.uint32) != want.view(np.uint32)).any(axis=2)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"
