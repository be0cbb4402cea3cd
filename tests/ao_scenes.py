"""The scenes and samplers of the AOIntegrator golden films (tests/golden/ao_*.npz, listed in ao_films.json): shared by
tools/make_golden_ao.py, which renders them with the real reference, and tests/test_ao.py / tests/test_ao_gpu.py."""

# name: (sampler kind, the sampler's count) -- the AO sample count is max(sampler.spp() / 8, 1)
AO_FILMS = {
    "cbox_readme_64_s64": ("blue", 64),
    "cbox_ragged_45x37_s16": ("blue", 16),
    "cbox_readme_24_s4": ("blue", 4),
    "zoo_48_s32": ("blue", 32),
    "xshapes_40_s16": ("blue", 16),
    "mesh_48_s32": ("blue", 32),
    "cones10k_32x16_s16": ("blue", 16),
    "sobol_cbox_32_s24": ("sobol", 24),
    "halton_zoo_32_s16": ("halton", 16),
    "lens_zoo_32_s16": ("blue", 16),
}


def _lens_zoo():
    import pine_amd as pa
    from pine_amd import scenes
    scene = scenes.shapes_zoo((32, 32))
    # the zoo's camera with a non-zero aperture: the lens sample is drawn before the pixel jitter
    scene.set(pa.ThinLenCamera(pa.Film([32, 32], pa.Uncharted2()), [0, 1, -4], [0, 1, 0], 0.25, 0.05, 4.0))
    return scene


def ao_scene(name):
    from pine_amd import scenes
    return {
        "cbox_readme_64_s64": lambda: scenes.cbox((64, 64), "readme"),
        "cbox_ragged_45x37_s16": lambda: scenes.cbox((45, 37), "committed"),
        "cbox_readme_24_s4": lambda: scenes.cbox((24, 24), "readme"),
        "zoo_48_s32": lambda: scenes.shapes_zoo((48, 48)),
        "xshapes_40_s16": lambda: scenes.xshapes_zoo((40, 40), extra_lights=False),
        "mesh_48_s32": lambda: scenes.sss((48, 48), 2),
        "cones10k_32x16_s16": lambda: scenes.classic_cones((32, 16), 100),
        "sobol_cbox_32_s24": lambda: scenes.cbox((32, 32), "readme"),
        "halton_zoo_32_s16": lambda: scenes.shapes_zoo((32, 32)),
        "lens_zoo_32_s16": _lens_zoo,
    }[name]()


def ao_sampler(name):
    import pine_amd as pa
    kind, spp = AO_FILMS[name]
    return {"blue": pa.BlueSampler, "sobol": pa.SobolSampler, "halton": pa.HaltonSampler}[kind](spp)
