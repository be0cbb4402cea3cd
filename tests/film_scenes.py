"""The scenes the pine-order golden films (tests/golden/film_*) were rendered from, and the sampler each was rendered with:
shared by tests/test_gpu_parity.py and tests/test_kernel_matrix.py."""


def film_scene(name):
    """FILM_NAMES, SOBOL_FILM_NAMES and HALTON_FILM_NAMES (conftest.py) -> the scene."""
    import pine_amd as pa
    from pine_amd import scenes
    return {
        "cbox_committed_64_s16_d4": lambda: scenes.cbox((64, 64), "committed"),
        "cbox_readme_64_s16_d4": lambda: scenes.cbox((64, 64), "readme"),
        "cbox_readme_64_s256_d8": lambda: scenes.cbox((64, 64), "readme"),
        "cbox_rect_readme_64_s64_d5": lambda: scenes.cbox((64, 64), "readme", False),
        "cbox_committed_ragged_45x37_s8_d3": lambda: scenes.cbox((45, 37), "committed"),
        "cbox_readme_64_s1_d1": lambda: scenes.cbox((64, 64), "readme"),
        "zoo_48_s16_d5": lambda: scenes.shapes_zoo((48, 48)),
        "classic_cones12_90x45_s32_d6": lambda: scenes.classic_cones((90, 45), 12),
        "sss_48_s32_d8": lambda: scenes.sss((48, 48), 1),
        "mats_zoo_64_s32_d6": lambda: scenes.materials_zoo((64, 64)),
        "classic_checker_cones8_90x45_s32_d6": lambda: scenes.classic_cones((90, 45), 8, checker_floor=True),
        "lights_zoo_64_s32_d6": lambda: scenes.lights_zoo((64, 64)),
        "lights_nosky_48_s16_d4": lambda: scenes.lights_zoo((48, 48), with_sky=False),
        "xshapes_48_s16_d5": lambda: scenes.xshapes_zoo((48, 48)),
        "xshapes_nolights_40_s8_d3": lambda: scenes.xshapes_zoo((40, 40), extra_lights=False),
        "mesh_glossy_48_s32_d6": lambda: scenes.sss((48, 48), 2, skin=pa.Glossy([0.9, 0.5, 0.3], 0.15), emissive_mesh=True),
        "sobol_cbox_readme_48_s8_d4": lambda: scenes.cbox((48, 48), "readme"),
        "sobol_cbox_ragged_45x37_s12_d3": lambda: scenes.cbox((45, 37), "committed"),
        "sobol_mats_zoo_32_s16_d6": lambda: scenes.materials_zoo((32, 32)),
        "sobol_cbox_readme_24_s512_d5": lambda: scenes.cbox((24, 24), "readme"),
        "sobol_sss_32_s8_d6": lambda: scenes.sss((32, 32), 2),
        "halton_cbox_readme_40_s8_d4": lambda: scenes.cbox((40, 40), "readme"),
        "halton_mats_zoo_32_s12_d6": lambda: scenes.materials_zoo((32, 32)),
        "halton_sss_24x20_s12_d5": lambda: scenes.sss((24, 20), 1, camera="committed"),
    }[name]()


def film_sampler(name, spp):
    """The sampler argument of pa.Plan for that film: SobolSampler / HaltonSampler, else BlueSampler's spp."""
    import pine_amd as pa
    if name.startswith("sobol_"):
        return pa.SobolSampler(spp)
    if name.startswith("halton_"):
        return pa.HaltonSampler(spp)
    return spp
