"""SURVEY.md 8(f) rank 4, mesh import: pine_amd/gltf.py against the reference's own importer.  tests/golden/import_test.glb
(written by tools/make_test_glb.py: node hierarchy with matrix / TRS, u16 and u32 indices, normals, texcoords, Uber
materials with ior / transmission / metallic, an emissive-strength lamp, a camera node) was imported AND rendered by the
real reference (`pine_ref gltf`, tools/make_golden.py --gltf); the scene this importer builds must render to the same
film, bit for bit -- on the CPU restatement here, on the MI355X in the -m gpu leg."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

GLB = os.path.join(GOLDEN, "import_test.glb")


def _scene():
    from pine_amd import gltf
    return gltf.load(GLB)


def test_import_builds_what_the_reference_imports(oracle):
    want = json.load(open(os.path.join(GOLDEN, "gltf_import.json")))["s4_d5"]
    sc = _scene()
    assert list(sc.camera.film().size) == want["size"]
    d = sc.describe()
    assert d.count("\nshape mesh") == want["geometries"] and d.count("shape mesh_full") == 6  # six primitives carry normals or texcoords
    assert d.count("material") >= 5 and " emissive " in d and " uber " in d
    film, _ = oracle.render(d, tuple(want["size"]), want["spp"], want["depth"])
    assert hashlib.md5(film.tobytes()).hexdigest() == want["md5"]
    np.testing.assert_array_equal(film[320, ::64, :3].reshape(-1), np.float32(want["row_320"]))


def test_import_errors():
    import pine_amd as pa
    from pine_amd import gltf
    with pytest.raises((pa.PineError, FileNotFoundError)):
        gltf.load(os.path.join(GOLDEN, "no_such_file.glb"))
    with pytest.raises(pa.PineError, match="normals"):
        pa.Mesh(np.zeros((3, 3), np.float32), [[0, 1, 2]], normals=np.zeros((2, 3), np.float32))


def test_mesh_apply_matches_the_reference_operand_order():
    """Mesh::apply (geometry.cpp:647-653): v = m * v, n = normalize(transpose(inverse(mat3(m))) * n) -- a pure scale leaves
    normals pointing the same way, a rotation rotates them, a non-uniform scale bends them away from the stretched axis."""
    import ctypes as C
    from pine_amd import _lib
    v = np.float32([[1, 2, 3], [0, 0, 0]])
    n = np.float32([[0, 0, 1], [1, 1, 0]] / np.float32(1.0))
    n[1] /= np.float32(np.sqrt(2))
    m = _lib.f16()
    _lib.lib.pine_gpu_mat4_scale(_lib.f3(2.0, 1.0, 1.0), m)
    _lib.check(_lib.lib.pine_gpu_mesh_apply(v.ctypes.data_as(_lib.c_f_p), 2, n.ctypes.data_as(_lib.c_f_p), m))
    np.testing.assert_array_equal(v[0], np.float32([2, 2, 3]))
    np.testing.assert_array_equal(n[0], np.float32([0, 0, 1]))
    assert n[1][0] < n[1][1] and abs(float(np.linalg.norm(n[1])) - 1) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["queue", "mega"])
def test_imported_scene_on_the_gpu_equals_the_reference(kernel, monkeypatch):
    import torch
    import pine_amd as pa
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    for key in ("s4_d5", "s16_d6"):
        want = json.load(open(os.path.join(GOLDEN, "gltf_import.json")))[key]
        sc = _scene()
        w, h = want["size"]
        plan = pa.Plan(sc, want["spp"], want["depth"], specialize=False)
        film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        plan.check()
        assert plan.stats().specialized == 0
        assert hashlib.md5(film.cpu().numpy().tobytes()).hexdigest() == want["md5"], key
        plan.close()


def _prl_load(extra=""):
    from pine_amd import prl
    out = prl.interpret(f'scene := Scene(); load(scene, "{GLB}"{extra}); integrator := PathIntegrator(BlueSampler(16), 6); '
                        'integrator.render(scene);', dry_run=True)
    return prl.scene_of_dry_run(out)


def test_prl_load_builtin_builds_the_same_scene():
    """`load(scene, "file.glb" [, mat4])` of the PRL front-end (fileio.cpp:584-589) goes through the C++ importer
    (pine_amd/host/gltf_import.hpp); pine_amd/gltf.py is pinned against the reference above, and the two must build the
    same scene, record for record -- camera included, with and without a global transform."""
    import pine_amd as pa
    from pine_amd import gltf, prl
    ps, spp, depth = _prl_load()
    assert (spp, depth) == (16, 6) and ps == _scene().describe()
    ps2, _, _ = _prl_load(", translate(0.5, 0.0, -0.25) * rotate_y(0.3)")
    assert ps2 == gltf.load(GLB, transform=pa.translate([0.5, 0.0, -0.25]) * pa.rotate_y(0.3)).describe() and ps2 != ps
    with pytest.raises(Exception, match="Unable to open"):
        prl.interpret('scene := Scene(); load(scene, "/no/such/file.glb");', dry_run=True)
    with pytest.raises(Exception):
        prl.interpret(f'scene := Scene(); load(scene, "{os.path.join(GOLDEN, "stats_640.json")}");', dry_run=True)  # not a glTF document


def _with_ties_overwritten(film, want):
    """The import scene has coplanar triangles of different meshes (a box standing on the floor); where a ray meets both at the same
    t Embree's own hierarchy -- not restated -- decides which it reports.  The fixture carries the reference's values at those 392
    pixels: a film equals the reference's everywhere else exactly when it has the reference's md5 after they are overwritten."""
    film = film.copy()
    for rec in want["tie_pixels"]:
        film[rec[0], rec[1]] = [float.fromhex(v) for v in rec[2:6]]
    return film


def test_oracle_in_embree_order_renders_the_embree_builds_film(oracle):
    want = json.load(open(os.path.join(GOLDEN, "gltf_import.json")))["embree_s4_d5"]
    sc = _scene()
    film, _ = oracle.render(sc.describe(), tuple(want["size"]), want["spp"], want["depth"], order="embree")
    assert len(want["tie_pixels"]) < 0.001 * film.shape[0] * film.shape[1]
    assert hashlib.md5(_with_ties_overwritten(film, want).tobytes()).hexdigest() == want["md5"]


@pytest.mark.gpu
def test_prl_load_renders_the_reference_film(monkeypatch):
    """A script's load() + PathIntegrator(sampler, n): the reference's default accel is EmbreeAccel -- the film of the reference
    built with Embree (every pixel but the coplanar ties, see above); $PINE_PRL_ACCEL=bvh: the film of the reference's own BVH."""
    from pine_amd import prl
    golden = json.load(open(os.path.join(GOLDEN, "gltf_import.json")))
    want = golden["s4_d5"]
    script = (f'scene := Scene(); load(scene, "{GLB}"); integrator := PathIntegrator(BlueSampler({want["spp"]}), {want["depth"]}); '
              'integrator.render(scene);')
    monkeypatch.delenv("PINE_PRL_ACCEL", raising=False)
    prl.interpret(script)
    emb = golden["embree_s4_d5"]
    assert hashlib.md5(_with_ties_overwritten(prl.last_film(), emb).tobytes()).hexdigest() == emb["md5"]
    monkeypatch.setenv("PINE_PRL_ACCEL", "bvh")
    prl.interpret(script)
    assert hashlib.md5(prl.last_film().tobytes()).hexdigest() == want["md5"]


def test_cpp_facade_load_builds_the_same_scene(tmp_path):
    """pine::load(scene, file [, mat4]) of the C++ facade (pine_amd/host/pine.hpp) is the same importer."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/pine_amd/host/pine.hpp"\n#include <cstdio>\n#include <vector>\n'
                   'int main(int, char** argv) {\n  pine::Scene s;\n  pine::load(s, argv[1]);\n'
                   '  std::vector<char> buf(1 << 20);\n  int n = pine_gpu_scene_describe(s.handle(), buf.data(), int(buf.size()));\n'
                   '  if (n < 0) return 2;\n  std::fwrite(buf.data(), 1, size_t(n), stdout);\n'
                   '  std::fprintf(stderr, "%%d %%d %%a", s.camera.film().size().x, s.camera.film().size().y, double(s.camera.fov));\n'
                   '  try { pine::load(s, "/no/such.glb"); } catch (const pine::Error&) { return 0; }\n  return 3;\n}\n' % root)
    exe = tmp_path / "t"
    lib = os.path.join(root, "pine_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O0", str(src), "-o", str(exe), "-L" + lib, "-lpine_gpu", "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([str(exe), GLB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc = _scene()
    assert r.stdout.rstrip("\x00") == sc.describe()
    w, h, fov = r.stderr.split()[-3:]
    assert [int(w), int(h)] == list(sc.camera.film().size) and float.fromhex(fov) == float(np.float32(sc.camera.fov))
