"""CPU: the precompiled path-kernel variants (pine_amd/csrc/pine_variants.h) as the library reports them
(pine_gpu_test_kernel_variants) against the matrix written out below.  tests/test_kernel_matrix.py renders every film
with every variant of this list: a variant added to or removed from the library fails here until the list -- and with
it the GPU matrix -- is updated on purpose."""
import ctypes as C

import numpy as np

# F_* feature bits (pine_amd/csrc/pine_device.h)
F = dict(AABB=1 << 0, OBB=1 << 1, SPHERE=1 << 2, DISK=1 << 3, CONE=1 << 4, MESH=1 << 5, UBER=1 << 6, SSS=1 << 7, LDS_SCENE=1 << 8,
         NODES=1 << 9, LIGHTS=1 << 10, XSHAPES=1 << 11, SOBOL=1 << 12, LDS_TOP=1 << 13, LDS_REST=1 << 14, XSTAGE=1 << 15,
         VLOG=1 << 16, BAKED=1 << 17, EMBREE=1 << 18)
ALL = 0xFF | F["NODES"] | F["LIGHTS"] | F["XSHAPES"] | F["SOBOL"]
BOXES = F["AABB"] | F["OBB"]
ANALYTIC = BOXES | F["SPHERE"] | F["DISK"] | F["CONE"] | F["UBER"]
NO_SSS = ALL & ~F["SSS"]
LDS_SCENE, LDS_TOP, LDS_REST, XSTAGE, VLOG, EMBREE = F["LDS_SCENE"], F["LDS_TOP"], F["LDS_REST"], F["XSTAGE"], F["VLOG"], F["EMBREE"]
QCTX = 1536  # PINE_QCTX: path contexts per workgroup of the scene-in-LDS stage-queued variants

# kind -> {order: (features, contexts per workgroup)}; order = position in the host's first-fit search
VARIANTS = {
    "queue": {
        0: (F["OBB"] | LDS_SCENE, QCTX),
        1: (BOXES | LDS_SCENE, QCTX),
        2: (ANALYTIC | LDS_SCENE, QCTX),
        3: (F["SPHERE"] | F["DISK"] | F["CONE"] | F["UBER"] | LDS_TOP, 1024),
        4: (ANALYTIC | LDS_TOP, 1024),
        5: (NO_SSS | LDS_REST | LDS_TOP | XSTAGE, 1024),
        6: (NO_SSS | LDS_REST | LDS_TOP, 1024),
        7: (NO_SSS | LDS_TOP | XSTAGE, 1024),
        8: (NO_SSS | LDS_TOP, 1024),
        9: (F["MESH"] | F["SSS"] | LDS_REST | LDS_TOP | XSTAGE, 1024),
        10: (F["MESH"] | F["SSS"] | LDS_REST | LDS_TOP, 1024),
        11: (ALL | LDS_REST | LDS_TOP | XSTAGE, 1024),
        12: (ALL | LDS_REST | LDS_TOP, 1024),
        13: (ALL | LDS_TOP | XSTAGE, 1024),
        14: (ALL | LDS_TOP, 1024),
        15: (ALL, 1024),                                 # 32-bit traversal stack, no node cache: the fallback of pine's order
        16: (F["OBB"] | LDS_SCENE | VLOG, QCTX),         # per-vertex log twins of 0 and 6
        17: (NO_SSS | LDS_REST | LDS_TOP | VLOG, 1024),
        18: (ANALYTIC | LDS_SCENE | EMBREE, QCTX),       # EmbreeAccel's order
        19: (ALL | EMBREE, 1024),                        # ... its fallback
    },
    "mega": {
        0: (BOXES | LDS_SCENE, 0),
        1: (ANALYTIC | LDS_SCENE, 0),
        2: (ANALYTIC, 0),
        3: (ALL | LDS_SCENE, 0),
        4: (ALL, 0),                                     # the fallback of pine's order
        5: (ALL | LDS_SCENE | EMBREE, 0),
        6: (ALL | EMBREE, 0),                            # ... of EmbreeAccel's order
    },
}
KIND = {"queue": 0, "mega": 1}


def library_variants(kind):
    """[(order, features, ctx)] of the library's table `kind` ("queue" / "mega"), in first-fit order."""
    from pine_amd import _lib
    n = _lib.check(_lib.lib.pine_gpu_test_kernel_variants(KIND[kind], None, None, None, 0), "kernel variants")
    features, ctx, order = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    got = _lib.lib.pine_gpu_test_kernel_variants(KIND[kind], features.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 ctx.ctypes.data_as(C.POINTER(C.c_int32)), order.ctypes.data_as(C.POINTER(C.c_int32)), n)
    assert got == n
    return [(int(o), int(f), int(c)) for o, f, c in zip(order, features, ctx)]


def test_the_compiled_variants_are_the_written_matrix():
    for kind, table in VARIANTS.items():
        assert library_variants(kind) == [(o, f, c) for o, (f, c) in sorted(table.items())], kind


def test_feature_sets_are_distinct_within_a_kind():
    """plan_stats.kernel_features then names the precompiled variant that ran."""
    for kind in VARIANTS:
        features = [f for _, f, _ in library_variants(kind)]
        assert len(set(features)) == len(features), kind


def test_the_enumeration_respects_its_capacity_and_checks_the_kind():
    from pine_amd import _lib
    first = np.full(3, 0xDEAD, np.uint32)
    n = _lib.lib.pine_gpu_test_kernel_variants(0, first.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, 2)
    assert n == len(VARIANTS["queue"])
    assert first.tolist() == [VARIANTS["queue"][0][0], VARIANTS["queue"][1][0], 0xDEAD]
    assert _lib.lib.pine_gpu_test_kernel_variants(2, None, None, None, 0) < 0
    assert "kind" in _lib.last_error()
