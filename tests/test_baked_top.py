"""CPU: the generated text of the one-mesh scenes of tests/baked_top_scenes.py (BakedForm::kTop): each
scene takes the top-level form, holds its mesh once, at the place the scene was built for, under the two-pass nodes it was
built for; the primitive limit; and one text compiles for gfx950 with the case ledger (-DPINE_TOP_CASES).
The films and the ledger itself: tests/test_baked_top_gpu.py."""
import ctypes as C
import os
import shutil

import pytest

import baked_top_scenes as B


@pytest.mark.parametrize("name", list(B.SCENES))
def test_scene_text_has_the_mesh_at_its_place(name):
    case = B.SCENES[name]
    texts = [B.source(B.build(name, cam)) for cam in B.CAMERAS]
    assert texts[0] == texts[1]  # (the kernel is keyed by geometry: the second camera costs no compile)
    text = texts[0]
    assert "#define PINE_BAKED_TOP 1" in text and "scene_traverse_baked_top" in text, f"{name}: not the top-level form"
    assert text.count("the mesh: traversed by the flat machine") == 1
    assert B.place(text) == case.place, (name, B.place(text))
    assert B.two_pass_ancestors(text) == case.two_pass, (name, B.two_pass_ancestors(text))
    assert ("swap01 =" in text) or not case.two_pass
    assert "mesh_reach" in text  # (the mesh-root gate is in the text)
    # a triangle may stand without a replay only in a top level of inline axis-aligned Rects (pine_queue_kernel.h)
    rects_only = text.count("const float denom = ") == len(case.place) - 1
    assert f"constexpr bool kBakedTopPlainRects = {'true' if rects_only else 'false'};" in text
    assert rects_only == (name != "scaled_box_after")
    assert set(case.reach) <= set(B.SLOTS) and 4 <= case.spp <= 16 and 1 <= case.depth <= 6
    assert all(24 <= n <= 32 for n in case.size)


def test_the_set_covers_every_place():
    places = {c.place for c in B.SCENES.values()}
    firsts = [p for p in places if p[0] == "M"]
    seconds = [p for p in places if p[1] == "M" and len(p) >= 7]
    lasts = [p for p in places if p[-1] == "M" and len(p) >= 7]
    middles = [p for p in places if "M" in p[2:-1] and len(p) >= 7]
    assert firsts and seconds and lasts and len(middles) >= 3, places
    assert any(len(c.place) <= 3 for c in B.SCENES.values())                  # a top level whose root is a leaf
    sides = {tuple(c.two_pass) for c in B.SCENES.values() if c.two_pass}
    assert (0,) in sides and (1,) in sides, sides                             # under a two-pass node, once in each child
    assert sum(c.depth == 1 for c in B.SCENES.values()) == 1                  # one scene of camera rays only
    assert {s for c in B.SCENES.values() for s in c.reach} >= {"replay_camera", "replay_spawned", "reached_with_hit", "tri_none_after"}


def test_primitive_limit():
    """Nine primitives and the mesh bake (ten instances); ten and the mesh decline."""
    import pine_amd as pa
    texts = []
    for n in (9, 10):
        s = B._limit(n)
        s.set(pa.ThinLenCamera(pa.Film([24, 24], pa.Uncharted2()), *B.CAMERAS["axis"]))
        texts.append(B.source(s))
    assert len(B.place(texts[0])) == 10 and B.place(texts[0]).count("M") == 1
    assert texts[1] == ""


def test_ledger_build_compiles_for_gfx950(tmp_path, monkeypatch):
    from pine_amd import _lib
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("PINE_GPU_SPECIALIZE_EXTRA", "-DPINE_TOP_CASES")
    out = C.create_string_buffer(1024)
    sc = B.build("inner_b_glossy")
    # the feature bits of pine_device.h, spelled out: a mesh scene whose traversal is a stage of its own -- the top form is emitted
    # for F_XSTAGE kernels only -- with the BSSRDF walk compiled in (the widest one-mesh variant; 1024 contexts as it has them)
    F_MESH, F_SSS, F_LDS_TOP, F_LDS_REST, F_XSTAGE = 1 << 5, 1 << 7, 1 << 13, 1 << 14, 1 << 15
    features, contexts = F_MESH | F_SSS | F_LDS_TOP | F_LDS_REST | F_XSTAGE, 1024
    assert _lib.lib.pine_gpu_test_specialize_compile(sc._h, features, contexts, b"gfx950", out, 1024) == 0, _lib.last_error()[-1500:]
    assert os.path.getsize(out.value.decode()) > 10000
    # ... and not together with the section profile, whose words it counts into
    monkeypatch.setenv("PINE_GPU_SPECIALIZE_EXTRA", "-DPINE_TOP_CASES -DPINE_PROFILE_SECTIONS")
    assert _lib.lib.pine_gpu_test_specialize_compile(sc._h, features, contexts, b"gfx950", out, 1024) < 0
    assert "PINE_TOP_CASES" in _lib.last_error()
