"""The scenes of the DenoiseIntegrator fixtures (tests/golden/denoise_*.npz): shared by tools/make_golden_denoise.py, which
renders them with the real reference, and tests/test_guides_gpu.py / test_denoise.py / test_denoise_gpu.py.

A film fixture holds albedo, normal (the reference's DenoiseIntegrator guide images), noisy (BlueSampler(16), pine-BVH order),
converged (SobolSampler(4096), same depth) and the .pscene text; a guides-only fixture holds albedo, normal and the text."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: max_path_length of the two films
DENOISE_FILMS = {
    "cbox_readme_64": 5,
    "mats_zoo_64": 5,
    "xshapes_48": 5,
    "sss_48": 6,
}
GUIDES_ONLY = ("cbox_ragged_45x37", "cbox_1x1", "cbox_8x1")
NOISY_SPP, CONVERGED_SPP = 16, 4096


def _xshapes_sky():
    import pine_amd as pa
    from pine_amd import scenes
    scene = scenes.xshapes_zoo((48, 48), extra_lights=False)
    scene.set(pa.Sky([0.9, 0.9, 1.0]))  # (an environment: the pixels that miss everything have a colour of their own)
    return scene


def denoise_scene(name):
    from pine_amd import scenes
    return {
        "cbox_readme_64": lambda: scenes.cbox((64, 64), "readme"),
        "mats_zoo_64": lambda: scenes.materials_zoo((64, 64)),  # Checkerboard and node-driven albedos: the node programs
        "xshapes_48": _xshapes_sky,
        "sss_48": lambda: scenes.sss((48, 48), 2),               # a mesh: triangle normals
        "cbox_ragged_45x37": lambda: scenes.cbox((45, 37), "committed"),
        "cbox_1x1": lambda: scenes.cbox((1, 1), "readme"),
        "cbox_8x1": lambda: scenes.cbox((8, 1), "readme"),
    }[name]()


def load(name):
    """The fixture as a dict of arrays (pscene: str)."""
    z = np.load(os.path.join(GOLDEN, f"denoise_{name}.npz"))
    d = {k: z[k] for k in z.files}
    d["pscene"] = bytes(d["pscene"]).decode()
    return d


def hits(normal):
    return (normal != 0).any(axis=2)
