"""GPU (-m gpu): EVERY precompiled path-kernel variant (pine_amd/csrc/pine_variants.h; the list is pinned by
tests/test_kernel_variants.py) against the reference's films, not only the one the first-fit search of plan creation
happens to pick.  PINE_GPU_TEST_VARIANT=queue:<order> / mega:<order> makes plan creation consider that variant alone;
PINE_GPU_TEST_LDS_NODES caps the LDS node cache of the F_LDS_TOP variants.  Every film is compared bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import (EMBREE_FILM_NAMES, EMBREE_MORE_FILM_NAMES, FILM_NAMES, HALTON_FILM_NAMES, SOBOL_FILM_NAMES, assert_bit_equal,
                      embree_scene, load_film)
from film_scenes import film_sampler, film_scene
from test_kernel_variants import F, VARIANTS

pytestmark = pytest.mark.gpu

PINE_FILMS = FILM_NAMES + SOBOL_FILM_NAMES + HALTON_FILM_NAMES
EMBREE_FILMS = EMBREE_FILM_NAMES + EMBREE_MORE_FILM_NAMES
ALL_FILMS = PINE_FILMS + EMBREE_FILMS
REFUSED = "pinned kernel variant does not cover this scene"
BLOCK = {"queue": 1024, "mega": 256}
# the variants that cover every scene of their order mode
FALLBACKS = {"pine": [("queue", 15), ("mega", 4)], "embree": [("queue", 19), ("mega", 6)]}
# plan-time knobs that would change what a plan picks: cleared for every test here
KNOBS = ("PINE_GPU_TEST_VARIANT", "PINE_GPU_TEST_LDS_NODES", "PINE_GPU_KERNEL", "PINE_GPU_NO_LDS_SCENE", "PINE_GPU_XSTAGE", "PINE_GPU_LDS_TRIS",
         "PINE_GPU_SPECIALIZE", "PINE_GPU_SPECIALIZE_FORCE", "PINE_GPU_SPECIALIZE_EXTRA")


def _clear(mp):
    for k in KNOBS:
        mp.delenv(k, raising=False)


def _film_case(name):
    """-> scene, sampler argument, depth, order mode, the fixture's film."""
    ref, ps, spp, depth = load_film(name)
    if name.startswith("embree_"):
        sc, sampler, order = embree_scene(name), spp, "embree"
    else:
        sc, sampler, order = film_scene(name), film_sampler(name, spp), "pine"
    assert sc.describe() == ps
    return sc, sampler, depth, order, ref


def _render(scene, spp, depth, **kw):
    import torch
    import pine_amd as pa
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, spp, depth, **kw)
    try:
        film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
        plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        plan.check()
        return film.cpu().numpy(), plan.stats()
    finally:
        plan.close()


def _pinned(mp, kind, vorder, scene, spp, depth, flags=0, **kw):
    """The film and stats of the precompiled variant kind:vorder, or None when plan creation refuses it as not covering the
    scene.  The per-vertex-log twins run with PINE_GPU_FLAG_VERTEX_LOG (the log itself stays off) -- in pine's order: the flag
    is refused with EmbreeAccel's, whose scenes those twins do not cover anyway.  kw: pa.Plan's."""
    import pine_amd as pa
    from pine_amd import _lib
    if VARIANTS[kind][vorder][0] & F["VLOG"] and kw.get("order", "pine") == "pine":
        flags |= _lib.FLAG_VERTEX_LOG
    mp.setenv("PINE_GPU_TEST_VARIANT", f"{kind}:{vorder}")
    try:
        return _render(scene, spp, depth, specialize=False, flags=flags, **kw)
    except pa.PineError as e:
        if REFUSED in str(e):
            return None
        raise
    finally:
        mp.delenv("PINE_GPU_TEST_VARIANT")


def _variant_of(st):
    kind = "queue" if st.block_threads == 1024 else "mega"
    (order,) = [o for o, (f, _) in VARIANTS[kind].items() if f == st.kernel_features]
    return kind, order


def _cell(mp, kind, order, sc, spp, depth, film_order, ref):
    """ok / refused / mismatch: ... / error: ..."""
    try:
        got = _pinned(mp, kind, order, sc, spp, depth, order=film_order)
    except Exception as e:  # (recorded: the test of this film fails with it)
        return f"error: {e}"
    if got is None:
        return "refused"
    film, st = got
    want = (VARIANTS[kind][order][0], BLOCK[kind], 0)
    have = (st.kernel_features, st.block_threads, st.specialized)
    if have != want:
        return f"mismatch: (kernel_features, block_threads, specialized) {have} != {want}"
    if film.shape != ref.shape:
        return f"mismatch: film shape {film.shape} != {ref.shape}"
    bad = (film.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    if bad.any():
        return f"mismatch: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    return "ok"


@pytest.fixture(scope="module")
def matrix():
    """Every film x every variant of both kernels: {(film, kind, order): cell}, {film: the unpinned plan's variant}, seconds."""
    cells, picks = {}, {}
    t0 = time.perf_counter()
    with pytest.MonkeyPatch.context() as mp:
        _clear(mp)
        for name in ALL_FILMS:
            sc, spp, depth, order, ref = _film_case(name)
            _, st = _render(sc, spp, depth, specialize=False, order=order)
            picks[name] = _variant_of(st)
            for kind, table in VARIANTS.items():
                for vorder in table:
                    cells[name, kind, vorder] = _cell(mp, kind, vorder, sc, spp, depth, order, ref)
    return cells, picks, time.perf_counter() - t0


def _table(cells):
    """The film x variant table: '#' rendered the fixture, '.' refused, 'X' mismatch, 'E' error; then films per variant."""
    cols = [(k, o) for k in VARIANTS for o in VARIANTS[k]]
    head = " " * 38 + " ".join(f"{k[0]}{o:<2}" for k, o in cols)
    mark = {"ok": "#", "refused": "."}
    rows = [f"{n:<38}" + " ".join(f"{mark.get(cells[n, k, o], cells[n, k, o][0].upper()):<3}" for k, o in cols) for n in ALL_FILMS]
    count = f"{'films rendered':<38}" + " ".join(f"{sum(cells[n, k, o] == 'ok' for n in ALL_FILMS):<3}" for k, o in cols)
    return "\n".join([head] + rows + [count])


@pytest.mark.parametrize("name", ALL_FILMS)
def test_every_variant_that_takes_a_film_renders_it_bit_for_bit(matrix, name):
    """(a) Each variant that accepts the scene renders the fixture bit for bit, reports its own feature set and workgroup size
    and runs unspecialised; a refusal is only ever the pinned-variant message."""
    cells, _, secs = matrix
    print(f"film x variant matrix: {secs:.1f} s")
    bad = {f"{k}:{o}": c for (n, k, o), c in cells.items() if n == name and c not in ("ok", "refused")}
    assert not bad, bad
    assert any(c == "ok" for (n, _, _), c in cells.items() if n == name)


def test_coverage_ledger(matrix):
    """(b) Every variant of both tables renders at least one film; the fallback variants take every film of their order mode;
    the variant an unpinned plan picks is among those that rendered the film."""
    cells, picks, _ = matrix
    table = _table(cells)
    print("\n" + table)
    problems = []
    for kind, variants in VARIANTS.items():
        for o in variants:
            if not any(cells[n, kind, o] == "ok" for n in ALL_FILMS):
                problems.append(f"{kind}:{o} renders no film")
    for mode, films in (("pine", PINE_FILMS), ("embree", EMBREE_FILMS)):
        for kind, o in FALLBACKS[mode]:
            problems += [f"{kind}:{o} (a fallback) does not render {n}: {cells[n, kind, o]}" for n in films if cells[n, kind, o] != "ok"]
    problems += [f"{n}: the unpinned plan picks {picks[n]}, which did not render it" for n in ALL_FILMS if cells[(n,) + picks[n]] != "ok"]
    assert not problems, "\n".join(problems) + "\n" + table


def test_pinning_errors(monkeypatch):
    import pine_amd as pa
    from pine_amd import _lib, scenes
    _clear(monkeypatch)
    sc = scenes.cbox((16, 16), "readme")
    for value, message in (("queue:99", "no such kernel variant"), ("mega:7", "no such kernel variant"), ("queue", "expected queue:<order>"),
                           ("sideways:1", "expected queue:<order>"), ("queue:-1", "expected queue:<order>")):
        monkeypatch.setenv("PINE_GPU_TEST_VARIANT", value)
        with pytest.raises(pa.PineError, match=message):
            pa.Plan(sc, 4, 3, specialize=False)
    monkeypatch.setenv("PINE_GPU_TEST_VARIANT", "queue:0")
    with pytest.raises(pa.PineError, match="not with PINE_GPU_FLAG_FAST"):
        pa.Plan(sc, 4, 3, flags=_lib.FLAG_FAST)
    # a pinned plan never specialises, even when asked to
    _, st = _render(sc, 4, 3, specialize=True)
    assert st.specialized == 0 and st.specialize_source == 0 and st.kernel_features == VARIANTS["queue"][0][0]
    monkeypatch.setenv("PINE_GPU_TEST_VARIANT", "queue:3")  # (no boxes)
    with pytest.raises(pa.PineError, match=REFUSED):
        pa.Plan(sc, 4, 3, specialize=False)


def _edge_scene(name):
    """-> scene, spp, depth: a top-level BVH alone, a top level and one mesh BVH, a top level and two mesh BVHs."""
    import pine_amd as pa
    from pine_amd import scenes
    return {"classic_cones12": lambda: (scenes.classic_cones((90, 45), 12), 8, 5),
            "sss_48": lambda: (scenes.sss((48, 48), 1), 8, 6),
            "mesh_glossy_48": lambda: (scenes.sss((48, 48), 2, skin=pa.Glossy([0.9, 0.5, 0.3], 0.15), emissive_mesh=True), 8, 6)}[name]()


@pytest.mark.parametrize("name", ["classic_cones12", "sss_48", "mesh_glossy_48"])
def test_node_cache_edge(oracle, monkeypatch, name):
    """(c) fetch_node reads nodes below the cached count from LDS and the rest from memory.  Every F_LDS_TOP variant that covers
    the scene, with the cache cut at 0, 1, 2, around the first mesh BVH's root (breadth-first numbering across the top level
    and the meshes), at half, and at and around the node count; triangle packets in LDS off and on.  lds_bytes shows that the
    cap applied: 64 bytes (one DNode) per cached node."""
    from pine_amd import _lib
    _clear(monkeypatch)
    sc, spp, depth = _edge_scene(name)
    w, h = sc.camera.film().size
    n = _lib.check(_lib.lib.pine_gpu_scene_build_accel(sc._h))
    bv = np.zeros(5 * 64, np.int32)
    nb = _lib.check(_lib.lib.pine_gpu_scene_accel_bvhs(sc._h, bv.ctypes.data_as(C.POINTER(C.c_int32)), bv.size))
    bv = bv[:5 * nb].reshape(nb, 5)
    caps = {0, 1, 2, n // 2, n - 1, n, n + 5}
    if nb > 1 and bv[1, 0] >= 0:
        root = int(bv[1, 0])
        caps |= {root - 1, root, root + 1}
    caps = sorted(c for c in caps if c >= 0)
    ref, _ = oracle.render(sc.describe(), (w, h), spp, depth)
    tried = []
    for order, (features, _) in VARIANTS["queue"].items():
        if not features & F["LDS_TOP"]:
            continue
        for tris in (("0", "1") if features & F["MESH"] else (None,)):
            if tris is None:
                monkeypatch.delenv("PINE_GPU_LDS_TRIS", raising=False)
            else:
                monkeypatch.setenv("PINE_GPU_LDS_TRIS", tris)
            monkeypatch.delenv("PINE_GPU_TEST_LDS_NODES", raising=False)
            full = _pinned(monkeypatch, "queue", order, sc, spp, depth)
            if full is None:
                break  # (the variant does not cover the scene)
            what = f"{name}, queue:{order}, PINE_GPU_LDS_TRIS={tris}"
            assert_bit_equal(full[0], ref, what + ", no cap")
            monkeypatch.setenv("PINE_GPU_TEST_LDS_NODES", "0")
            base = _pinned(monkeypatch, "queue", order, sc, spp, depth)[1].lds_bytes
            cached, rest = divmod(full[1].lds_bytes - base, 64)
            assert rest == 0 and 1 <= cached <= n, (what, full[1].lds_bytes, base)
            for cap in caps:
                monkeypatch.setenv("PINE_GPU_TEST_LDS_NODES", str(cap))
                film, st = _pinned(monkeypatch, "queue", order, sc, spp, depth)
                assert st.lds_bytes == base + 64 * min(cap, cached), (what, cap, st.lds_bytes, base, cached)
                assert_bit_equal(film, ref, f"{what}, {cap} of {n} nodes cached")
            tried.append((order, tris, cached))
    monkeypatch.delenv("PINE_GPU_TEST_LDS_NODES", raising=False)
    print(name, n, "nodes, caps", caps, "variants (order, LDS_TRIS, nodes cached uncapped)", tried)
    assert tried


def _baked_source(sc):
    from pine_amd import _lib
    n = _lib.lib.pine_gpu_scene_specialized_source(sc._h, None, 0)
    assert n >= 0, _lib.last_error()
    if n == 0:
        return ""
    buf = C.create_string_buffer(int(n) + 1)
    _lib.lib.pine_gpu_scene_specialized_source(sc._h, buf, n + 1)
    return buf.value.decode()


def test_scene_kernels_render_the_golden_films(monkeypatch, tmp_path_factory):
    """(d) The scene's own kernels (PINE_GPU_FLAG_SPECIALIZE), compiled into a cache private to this session, on every golden
    film of both order modes -- and the baked-eligible ones also with PINE_GPU_FLAG_SPECIALIZE_NO_BAKE: the fixture bit for
    bit.  Level 2 (baked) wherever the scene qualifies in pine's order, never in EmbreeAccel's order or without baking;
    level 1 is a strict subset of the precompiled variant's features; level 0 only where the precompiled variant already is the
    scene's exact feature set (checked by forcing the compile: PINE_GPU_SPECIALIZE_FORCE).  Films of one kernel share its
    compile through the cache."""
    from pine_amd import _lib
    _clear(monkeypatch)
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path_factory.mktemp("kernel_cache")))
    t0 = time.perf_counter()
    levels = {}
    for name in ALL_FILMS:
        sc, spp, depth, order, ref = _film_case(name)
        _, st0 = _render(sc, spp, depth, specialize=False, order=order)
        source = _baked_source(sc) if order == "pine" else ""
        # (no mesh: the whole scene as code; one mesh: its top level, on the traversal-stage variants only)
        bakes = bool(source) and ("PINE_BAKED_TOP" not in source or bool(st0.kernel_features & F["XSTAGE"]))
        runs = [("", 0)] + ([("no bake", _lib.FLAG_SPECIALIZE_NO_BAKE)] if bakes else [])
        for label, extra in runs:
            film, st = _render(sc, spp, depth, specialize=True, order=order, flags=extra)
            what = f"{name} ({order} order{', ' + label if label else ''})"
            assert_bit_equal(film, ref, what)
            levels[what] = st.specialized
            if bakes and not extra:
                assert st.specialized == 2 and st.kernel_features & F["BAKED"], (what, st.specialized)
            else:
                assert st.specialized in (0, 1), (what, st.specialized)
            if st.specialized == 1:
                assert st.kernel_features != st0.kernel_features and st.kernel_features & ~st0.kernel_features == 0, (what, hex(st.kernel_features))
            if st.specialized == 0:
                monkeypatch.setenv("PINE_GPU_SPECIALIZE_FORCE", "1")
                forced, stf = _render(sc, spp, depth, specialize=True, order=order, flags=_lib.FLAG_SPECIALIZE_NO_BAKE)
                monkeypatch.delenv("PINE_GPU_SPECIALIZE_FORCE")
                assert stf.specialized == 1 and stf.kernel_features == st0.kernel_features, (what, hex(stf.kernel_features), hex(st0.kernel_features))
                assert_bit_equal(forced, ref, what + ", forced exact feature set")
    print(f"scene kernels on {len(levels)} renders: {time.perf_counter() - t0:.1f} s", levels)


def test_shards_per_variant(monkeypatch):
    """(e) Every stage-queued variant that covers the Subsurface scene (tile classes, serial chains): three shards sum to the
    fixture bit for bit."""
    _clear(monkeypatch)
    name = "sss_48_s32_d8"
    sc, spp, depth, order, ref = _film_case(name)
    done = []
    for vorder in VARIANTS["queue"]:
        total = None
        for rank in range(3):
            got = _pinned(monkeypatch, "queue", vorder, sc, spp, depth, shard_rank=rank, shard_world=3)
            if got is None:
                break
            total = got[0] if total is None else total + got[0]
        if total is not None:
            assert_bit_equal(total, ref, f"{name}: queue:{vorder}, 3 shards")
            done.append(vorder)
    print("variants", done)
    assert len(done) >= 6, done
