"""The scenes of the strip films (tests/golden/film_strip_*): shared by tools/make_golden.py --draws and
tests/test_sampler_draws.py.  One pixel coordinate runs to 600 -- past HaltonSampler's and BlueSampler's 128-pixel wrap and past
a 512 Morton range -- while the other stays below 2."""

STRIP_FILM_NAMES = ["strip_sobol_600x2_s6_d4", "strip_sobol_2x600_s6_d4", "strip_halton_600x2_s6_d4", "strip_halton_2x600_s6_d4",
                    "strip_sobol_slit_600x2_s6_d4", "strip_halton_slit_600x2_s6_d4"]


def strip_scene(name):
    """-> (scene, sampler name, spp, depth).  `600x2` / `2x600`: scenes.cbox(size, "readme") as it is; the camera's field of view
    is that of the film's height, so the room fills the tall strip but only the four middle pixels of the wide one.  `slit`: the
    same room and camera with a field of view of 1 / 1024, which lays the room over 85 % of the 600 pixels."""
    import pine_amd as pa
    from pine_amd import scenes
    size = (2, 600) if "2x600" in name else (600, 2)
    scene = scenes.cbox(size, "readme")
    if "_slit_" in name:
        scene.set(pa.ThinLenCamera(pa.Film(list(size), pa.Uncharted2()), [0, 1, -4], [0, 1, 0], 1.0 / 1024))
    return scene, ("halton" if "_halton_" in name else "sobol"), 6, 4
