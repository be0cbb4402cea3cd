"""One-mesh scenes for the baked top level (BakedForm::kTop), with the mesh at every place in pine's order:
shared by tests/test_baked_top.py (the generated text), tests/test_baked_top_gpu.py (films and the case ledger),
tests/test_oracle_golden.py and tools/make_golden.py --baked-top (the three films the real reference rendered).

A scene's PLACE is its top level as the generated text stores it: one letter per primitive in order of appearance, `p` for a
primitive and `M` for the mesh.  Each entry of SCENES says what the scene is for, where its mesh must land, and which slots of
the case ledger (TopCase, pine_queue_kernel.h) at least 32 of its rays must reach under each of the two cameras."""
import numpy as np

# TopCase (pine_amd/csrc/pine_queue_kernel.h), by name
SLOTS = ["settled", "reached_miss", "reached_prim", "tri_none_after", "tri_in_front", "tri_tie", "replay_camera", "replay_spawned",
         "reached_with_hit", "shadow_top_occluded", "shadow_top_clear", "shadow_xs_occluded", "shadow_xs_clear",
         "parked_next_resolved", "parked_next_xc", "parked_no_next"]
CLOSEST = SLOTS[0:5] + SLOTS[6:8]   # one of these per closest-hit ray (tri_tie and reached_with_hit are counted besides)
SHADOW = SLOTS[9:13]                # one of these per shadow ray
PARKED = SLOTS[13:16]               # one of these per vertex whose shadow ray went to stage XS

LAMP = (np.float32(600) * np.array([1.0, 0.64, 0.185], dtype=np.float32)).tolist()
WALLS = {"floor": ([0, 0, 1], [2, 0, 0], [0, 0, 2], True, "floor"), "ceiling": ([0, 2, 1], [2, 0, 0], [0, 0, 2], False, "floor"),
         "left": ([-1, 1, 1], [0, 0, 2], [0, 2, 0], True, "red"), "right": ([1, 1, 1], [0, 0, 2], [0, 2, 0], False, "green"),
         "back": ([0, 1, 2], [2, 0, 0], [0, 2, 0], True, "blue")}
ALL_WALLS = ("floor", "ceiling", "left", "right", "back")
# the camera on the axis of the room (rays with zero components) and one off it
CAMERAS = {"axis": ([0, 1, -4], [0, 1, 0], 0.25), "off": ([0.7, 1.45, -3.1], [-0.15, 0.8, 1.0], 0.3)}


def loose_triangles(points):
    """A mesh of separate triangles: `points` is (n, 3, 3)."""
    v = np.float32(points).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


def shard_fan(centre, reach, n, seed):
    """n loose triangles around `centre`, their corners within `reach` of it on each axis."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)
    mid = c + rng.uniform(-1, 1, (n, 1, 3)) * np.asarray(reach) * 0.7
    return loose_triangles(mid + rng.uniform(-1, 1, (n, 3, 3)) * np.asarray(reach) * 0.45)


def _room(walls=ALL_WALLS, lamp=True):
    import pine_amd as pa
    s = pa.Scene()
    s.add("floor", pa.Diffuse([0.9, 0.9, 0.9]))
    s.add("blue", pa.Diffuse([0.2, 0.5, 0.9]))
    s.add("red", pa.Diffuse([0.9, 0.1, 0.05]))
    s.add("green", pa.Diffuse([0.2, 0.9, 0.05]))
    for w in walls:
        pos, ex, ey, flip, mat = WALLS[w]
        s.add(pa.Rect(pos, ex, ey, flip), mat)
    if lamp:
        s.add(pa.Rect([0.0, 1.9, 1], [0.1, 0, 0], [0, 0, 0.1]), pa.Emissive(LAMP))
    return s


def _ico(centre, radius=0.15, level=1):
    from pine_amd.scenes import icosphere
    return icosphere(level, radius, centre)


def _skin(kind):
    import pine_amd as pa
    return {"diffuse": lambda: pa.Diffuse([0.8, 0.7, 0.3]), "glossy": lambda: pa.Glossy([0.9, 0.5, 0.3], 0.15),
            "emissive": lambda: pa.Emissive([30.0, 24.0, 12.0]), "sss": lambda: pa.Subsurface([1, 1, 1], 0.0, [40, 40, 40])}[kind]()


def _plain(centre, radius=0.15, skin="diffuse", walls=ALL_WALLS):
    def build():
        import pine_amd as pa
        s = _room(walls)
        v, f = _ico(centre, radius)
        s.add(pa.Mesh(v, f), _skin(skin))
        return s
    return build


def _scaled_box_after():
    import pine_amd as pa
    s = _room()
    v, f = _ico((0.0, 1.0, 0.2), 0.2)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    # a scaled Box(AABB, mat4) that cuts into the sphere's right half from the front: its answer depends on the tmax it is
    # tested with, and rays from the cameras meet it before the triangle behind it
    s.add(pa.Box(pa.AABB([0, 0, 0], [1, 1, 1]), pa.translate([0.05, 0.8, -0.1]) * pa.scale([0.4, 0.45, 0.3])), "green")
    return s


def _through_wall():
    import pine_amd as pa
    s = _room()
    # loose triangles through the right wall (x = 1), half of them inside the room: triangle and Rect hits interleave along a ray
    v, f = shard_fan((1.0, 0.4, 0.5), (0.3, 0.3, 0.4), 24, 11)
    s.add(pa.Mesh(v, f), _skin("glossy"))
    return s


def _camera_inside():
    import pine_amd as pa
    s = _room()
    # loose triangles from behind the cameras into the room: both cameras sit inside the mesh's bounding box
    v, f = shard_fan((0.2, 1.1, -1.6), (1.0, 0.8, 3.2), 40, 12)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    return s


def _outside():
    import pine_amd as pa
    s = _room()
    # behind the back wall (z = 2), seen by no camera ray: every triangle a ray finds lies behind a wall stored after the mesh
    v, f = _ico((0.3, 1.2, 2.5), 0.4)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    return s


def _ties():
    import pine_amd as pa
    s = _room()
    # two Rects in the plane z = 1 in front of the cameras' axis, one added before the mesh and one after (pine's order stores
    # both after it), and loose triangles IN that plane over both (and a few off it, so that the mesh's BVH has inner nodes):
    # rays meet triangle and Rect at one distance, up to the rounding of two different formulas -- measured: 350 exact ties
    # per film (r_pa == t_M: the triangle stands, as the reference's `t < tmax` rejects the Rect)
    s.add(pa.Rect([0.0, 1.0, 1.0], [0.5, 0, 0], [0, 0.5, 0], True), "red")
    tris = [[[-0.6, 0.6, 1.0], [0.6, 0.6, 1.0], [-0.6, 1.4, 1.0]], [[0.6, 0.6, 1.0], [0.6, 1.4, 1.0], [-0.6, 1.4, 1.0]]]
    rng = np.random.default_rng(13)
    for _ in range(18):
        c = rng.uniform([-0.7, 0.3, 0.6], [0.7, 1.7, 1.6])
        tris.append((c + rng.uniform(-0.2, 0.2, (3, 3))).tolist())
    v, f = loose_triangles(tris)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    s.add(pa.Rect([0.5, 1.0, 1.0], [0.5, 0, 0], [0, 0.5, 0], True), "green")
    return s


def _limit(n_primitives):
    """`n_primitives` top-level primitives plus the mesh: the lamp, the five walls, and small Rects on the floor."""
    import pine_amd as pa
    s = _room()
    for k in range(n_primitives - 6):
        s.add(pa.Rect([-0.75 + 0.5 * k, 0.05 + 0.01 * k, 0.5], [0.2, 0, 0], [0, 0, 0.2], True), "red")
    v, f = _ico((0.0, 1.0, 1.0), 0.3)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    return s


def _root_leaf():
    import pine_amd as pa
    s = _room(("floor",))  # floor, lamp, mesh: three primitives, the top level's root is a leaf
    v, f = _ico((0.1, 0.9, 0.9), 0.45)
    s.add(pa.Mesh(v, f), _skin("diffuse"))
    return s


class Case:
    def __init__(self, make, place, two_pass, spp, depth, reach, purpose, size=(24, 24)):
        self.make, self.place, self.two_pass, self.spp, self.depth, self.reach, self.purpose, self.size = make, place, two_pass, spp, depth, reach, purpose, size


# place: the mesh's place in the generated text; two_pass: the two-pass nodes (`swap01`) above the mesh, outermost first, 0 / 1 =
# the mesh is in the node's first / second child; reach: the ledger slots at least 32 rays of the scene must take under each
# camera -- what the scene is for; the floor is a condition on the scene, not a result
SCENES = {
    "first_depth1": Case(_plain((0.0, 1.0, 0.2)), "Mpppppp", [], 16, 1, ["settled", "tri_in_front"],
                         "mesh first, camera rays only: the closest-hit slots sum to W * H * spp", (32, 32)),
    "outside_first": Case(_outside, "Mpppppp", [], 8, 5, ["replay_camera", "replay_spawned"],
                          "mesh outside the room behind the back wall, stored first: every triangle found lies behind a wall accepted after the mesh"),
    "second_through_back": Case(_plain((0.0, 1.0, 2.0), 0.3), "pMppppp", [], 8, 4, ["reached_with_hit", "tri_in_front"],
                                "mesh second, a sphere half through the back wall: one primitive before it, five after"),
    "inner_a_sss": Case(_plain((0.75, 0.25, 0.3), 0.2, "sss"), "pppMppp", [0], 16, 6, ["reached_with_hit", "parked_next_xc"],
                        "Subsurface mesh in the middle, under a node with two inner children: walk stage and sample tokens on the baked top level", (32, 32)),
    "inner_b_glossy": Case(_plain((-0.75, 0.25, 0.3), 0.2, "glossy"), "ppppMpp", [0], 16, 5, ["reached_with_hit", "shadow_xs_occluded"],
                           "mesh fifth of seven under a node with two inner children: rays reach it with a hit recorded and a shortened tmax", (32, 32)),
    "through_wall": Case(_through_wall, "pppppMp", [1], 16, 5, ["reached_with_hit", "reached_prim", "replay_camera", "replay_spawned"],
                         "loose triangles through the right wall, in the SECOND child of a two-pass node: triangle and Rect hits interleave", (32, 32)),
    "last": Case(_plain((0.6, 1.7, 0.4), 0.25), "ppppppM", [], 16, 4, ["tri_none_after", "reached_with_hit"],
                 "mesh LAST: nothing is stored after it, r_pb == 0 on every ray", (32, 32)),
    "middle_emissive": Case(_plain((0.0, 1.8, 1.0), 0.3, "emissive"), "ppppMpp", [], 8, 4, ["shadow_xs_clear", "shadow_xs_occluded"],
                            "an emissive mesh through the ceiling and around the lamp, the only other light: shadow rays to the mesh end on it, those to the lamp are stopped by it"),
    "root_leaf": Case(_root_leaf, "ppM", [], 8, 4, ["reached_miss", "tri_none_after"],
                      "floor, lamp and mesh: the top level's root is itself a leaf; most rays miss everything"),
    "open_two_walls": Case(_plain((-0.6, 0.4, 0.5), 0.25, walls=("floor", "left")), "ppMp", [], 16, 5, ["reached_miss", "settled", "tri_none_after"],
                           "two walls only: mesh hits with nothing behind them, many rays miss everything", (32, 32)),
    "camera_inside": Case(_camera_inside, "Mpppppp", [], 8, 4, ["reached_prim", "tri_in_front"],
                          "loose triangles from behind the cameras into the room: the cameras sit inside the mesh's bounding box"),
    "scaled_box_after": Case(_scaled_box_after, "Mppppppp", [], 16, 5, ["replay_camera", "replay_spawned"],
                             "a scaled Box(AABB, mat4) stored after the mesh and cutting into it: the shape whose answer depends on tmax -- "
                             "every triangle hit is replayed (kBakedTopPlainRects is false)", (32, 32)),
    "ties": Case(_ties, "Mpppppppp", [], 8, 4, ["tri_in_front", "tri_tie"],
                 "triangles coplanar with two axis-aligned Rects stored after the mesh: triangle and Rect at exactly one distance, the triangle stands"),
}
# the three films the REAL reference rendered (tools/make_golden.py --baked-top -> tests/golden/film_<name>.npz): axis camera, 24 x 24
GOLDEN_FILMS = {"baked_top_last_24_s16_d4": "last", "baked_top_inner_b_glossy_24_s16_d5": "inner_b_glossy", "baked_top_scaled_box_after_24_s16_d5": "scaled_box_after"}


def build(name, camera="axis", size=None):
    import pine_amd as pa
    case = SCENES[name]
    scene = case.make()
    frm, to, fov = CAMERAS[camera]
    scene.set(pa.ThinLenCamera(pa.Film(list(size or case.size), pa.Uncharted2()), frm, to, fov))
    return scene


def source(scene):
    """The text generated for the scene ("" when it does not qualify)."""
    import ctypes as C
    from pine_amd import _lib
    n = _lib.lib.pine_gpu_scene_specialized_source(scene._h, None, 0)
    assert n >= 0, _lib.last_error()
    if n == 0:
        return ""
    buf = C.create_string_buffer(n + 1)
    assert _lib.lib.pine_gpu_scene_specialized_source(scene._h, buf, n + 1) == n
    return buf.value.decode()


def place(text):
    """The top level as the text stores it: every primitive assigns geom_out once; the mesh does so in its MODE 1 line."""
    return "".join("M" if "m.t < ray.tmax" in ln else "p" for ln in text.splitlines() if "geom_out = " in ln)


def two_pass_ancestors(text):
    """The two-pass nodes (both children inner: `swap01`) above the mesh, outermost first: 0 where the mesh lies in the
    node's first child, 1 where in its second."""
    lines = text.splitlines()
    indent = lambda ln: len(ln) - len(ln.lstrip())
    at = next(i for i, ln in enumerate(lines) if "m.t < ray.tmax" in ln)
    level, found = indent(lines[at]), []
    for ln in reversed(lines[:at]):
        if indent(ln) < level and ln.strip():
            level = indent(ln)
            if "== swap01) {" in ln:
                found.append(0 if "if (in0 &&" in ln else 1)
    return found[::-1]
