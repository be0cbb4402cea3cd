"""CPU: Shader's batched path-vertex queries (include/pine_gpu.h pine_gpu_shader_*) as far as a machine without a GPU can see
them -- the symbols and their ctypes signatures, the layout call against the Python constants, creation failing loudly, the
ValueError paths of the Python wrappers on CPU tensors, pine::Shader compiling, the example importing.  The kernels are
tested on the GPU in tests/test_shader_gpu.py."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["pine_gpu_shader_create", "pine_gpu_shader_destroy", "pine_gpu_shader_layout", "pine_gpu_shader_info", "pine_gpu_shader_begin_device",
         "pine_gpu_shader_vertex_device", "pine_gpu_shader_fold_device", "pine_gpu_shader_resolve_device"]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_symbols_exist_and_are_declared():
    from pine_amd import _lib
    header = open(os.path.join(ROOT, "include", "pine_gpu.h")).read()
    for n in NAMES:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SIGNATURES and n + "(" in header, n


def test_layout_agrees_with_the_python_constants():
    from pine_amd import _lib, api
    out = (C.c_int32 * 4)(-1, -1, -1, -1)
    assert _lib.lib.pine_gpu_shader_layout(out) == 0
    state, record, ray, log = (int(x) for x in out)
    assert (state, record, ray, log) == (4 * api.SHADER_STATE_WORDS, 4 * api.SHADER_RECORD_WORDS, api.SHADER_RAY_FLOATS, api.SHADER_LOG_FLOATS)
    assert state % 16 == 0 and record % 16 == 0 and (4 * ray) % 16 == 0 and (4 * log) % 16 == 0
    assert api.RECORD_DTYPE.itemsize == record and api.HIT_DTYPE.itemsize == 48
    assert _lib.lib.pine_gpu_shader_layout(None) < 0 and "null" in _lib.last_error()


def test_create_without_a_gpu_fails_with_a_message():
    """No GPU: a message, no crash, nothing approximated on the CPU.  (Where there is one, creation succeeds.)"""
    import pine_amd as pa
    from pine_amd import scenes
    if not _no_gpu():
        with pa.Shader(scenes.cbox((8, 8), "readme"), pa.BlueSampler(4), 3) as sh:
            assert sh.film_size == (8, 8) and sh.spp == 4
        return
    with pytest.raises(pa.PineError, match="no HIP device available: Shader"):
        pa.Shader(scenes.cbox((8, 8), "readme"), pa.BlueSampler(4), 3)
    with pytest.raises(pa.PineError, match="no HIP device"):
        pa.WavefrontPathIntegrator(pa.BlueSampler(4), 3).render(scenes.cbox((8, 8), "readme"))


def test_refusals_that_need_no_gpu_name_their_cause():
    """What is refused before the device is looked at: a flag bit, shards, a Subsurface material (by name), a bad depth or
    sample count, null arguments."""
    import pine_amd as pa
    from pine_amd import _lib, scenes
    sc = scenes.cbox((8, 8), "readme")
    for flag, word in ((_lib.FLAG_FAST, "FLAG_FAST"), (_lib.FLAG_SPECIALIZE, "FLAG_SPECIALIZE"), (_lib.FLAG_VERTEX_LOG, "FLAG_VERTEX_LOG"),
                       (_lib.FLAG_ORDER_EMBREE, "FLAG_ORDER_EMBREE"), (_lib.FLAG_TIMING, "no flag applies")):
        with pytest.raises(pa.PineError, match=word):
            pa.Shader(sc, pa.BlueSampler(4), 3, flags=flag)
    prm = _lib.RenderParams(4, 3, 0, 0, 2, 0, 0, 0)
    assert not _lib.lib.pine_gpu_shader_create(sc._h, C.byref(prm)) and "shard_world" in _lib.last_error()
    with pytest.raises(pa.PineError, match="Subsurface material `skin`"):
        pa.Shader(scenes.sss((8, 8), 1), pa.BlueSampler(4), 3)
    with pytest.raises(pa.PineError, match="max_path_length"):
        pa.Shader(sc, pa.BlueSampler(4), 0)
    with pytest.raises(pa.PineError, match="supported depth"):
        pa.Shader(sc, pa.BlueSampler(4), 33)
    with pytest.raises(pa.PineError, match="at most 4096"):
        pa.Shader(sc, pa.SobolSampler(4097), 3)
    with pytest.raises(pa.PineError, match="positive"):
        pa.Shader(sc, pa.SobolSampler(0), 3)
    assert not _lib.lib.pine_gpu_shader_create(None, C.byref(prm)) and "null" in _lib.last_error()
    assert _lib.lib.pine_gpu_shader_vertex_device(None, None, None, 4, None, None, None, None, None) < 0 and "null" in _lib.last_error()
    assert _lib.lib.pine_gpu_shader_info(None, None) < 0
    _lib.lib.pine_gpu_shader_destroy(None)  # (as free(NULL))


def _unbound_shader(w=4, h=4):
    """A Shader object without a handle: the wrappers check their tensors before they look at it."""
    from pine_amd import api
    sh = api.Shader.__new__(api.Shader)
    sh._h, sh.device, sh.film_size, sh.spp, sh.max_path_length = None, 0, (w, h), 4, 3
    return sh


def test_wrappers_raise_value_error_before_anything_is_launched():
    """Wrong dtype, shape, layout, device (a CPU tensor) or type: ValueError, and the handle is never reached."""
    import torch
    import pine_amd as pa
    sh = _unbound_shader()
    n = 16
    rays, hits = torch.zeros((n, 8)), torch.zeros((n, 12))
    states = torch.zeros((n, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        sh.begin(0, states, rays)
    with pytest.raises(ValueError, match="states of the sample before"):
        sh.begin(1)
    for bad_states in (states.float(), states[:, :7], states[:8], np.zeros((n, 8), np.int32)):
        with pytest.raises(ValueError):
            sh.begin(0, bad_states, rays)
    for bad_rays in (rays.double(), rays[:, :7], rays.reshape(-1), rays.repeat(1, 2)[:, ::2], None, rays):
        with pytest.raises(ValueError):
            sh.vertex(bad_rays, hits, states)
    with pytest.raises(ValueError):
        sh.vertex(rays, hits[:, :11], states)
    records, occluded, sums = torch.zeros((3, n, 16)), torch.zeros((3, n), dtype=torch.uint8), torch.zeros((n, 4))
    for args in ((records[:, :, :15], occluded, 0, sums), (records, occluded.float(), 0, sums), (records, occluded[:2], 0, sums),
                 (records, occluded, 0, sums[:, :3]), (records, occluded, 0, sums, torch.zeros((3, n, 15))), (records, occluded, 0, sums)):
        with pytest.raises(ValueError):
            sh.fold(*args)
    for args in ((sums[:, :3],), (sums.double(),), (sums, torch.zeros((n + 1, 4))), (sums,)):
        with pytest.raises(ValueError):
            sh.resolve(*args)
    with pytest.raises(pa.PineError, match="camera"):
        _unbound_shader(0, 0).begin(0)


def test_cpp_facade_compiles(tmp_path):
    """pine::Shader (pine_amd/host/pine.hpp) with every _device call: compiled and linked, not run."""
    src = tmp_path / "shader.cpp"
    src.write_text('''#include "pine.hpp"
int main(int argc, char**) {
  if (argc < 100) return 0;  // (compiled and linked only)
  pine::Scene scene;
  pine::Shader shader(scene, pine::BlueSampler(4), 3);
  static_assert(pine::Shader::state_bytes == 32 && pine::Shader::record_bytes == sizeof(pine::VertexRecord), "layout");
  void* p = nullptr;
  shader.begin_device(0, p, p);
  shader.vertex_device(p, p, 0, p, p, p, p);
  shader.fold_device(p, p, 1, 0, 0, p);
  shader.resolve_device(p, 0, p);
  return shader.spp() + shader.film_width() + shader.film_height() + shader.max_path_length() + (shader.handle() != nullptr);
}
''')
    lib_dir = os.path.join(ROOT, "pine_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "pine_amd", "host"), str(src), "-L" + lib_dir, "-lpine_gpu",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "shader")])
    assert subprocess.run([str(tmp_path / "shader")], timeout=60).returncode == 0


def test_example_imports():
    spec = importlib.util.spec_from_file_location("wavefront_path", os.path.join(ROOT, "examples", "wavefront_path.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.render) and callable(mod.main)
