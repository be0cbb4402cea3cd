#!/usr/bin/env python3
"""examples/wavefront_path.py -- the Cornell box through WavefrontPathIntegrator: PathIntegrator's film, bit for bit, from a
loop over Accel's ray queries and Shader's vertex queries (pine_amd/api.py), plus an AOV the fused kernel cannot give -- the
albedo at the first hit, taken from the loop's per-level callback.

    begin -> intersect -> vertex -> hit -> intersect -> vertex -> ... -> fold -> resolve      (every sample, every level)

The callback sees the rays, Accel's hits and the vertex records of every level as device tensors.  A Diffuse surface's BSDF
value is albedo / pi whatever the direction, so the first level's `f` times pi IS the albedo; lamps and misses stay black.

    python examples/wavefront_path.py [size] [spp] [out.png] [albedo.png]
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import pine_amd as pa  # noqa: E402
from pine_amd import scenes  # noqa: E402
from pine_amd.api import KIND_SHADED  # noqa: E402


def render(size=64, spp=16, max_path_length=4, order="pine", device=0):
    """-> (film, albedo): two (size, size, 4) numpy arrays; the albedo is the mean over the samples of the first hit's."""
    scene = scenes.cbox((size, size), "readme")
    integrator = pa.WavefrontPathIntegrator(pa.BlueSampler(spp), max_path_length, order=order, device=device)
    total = torch.zeros((size * size, 3), dtype=torch.float32, device=torch.device("cuda", device))
    samples = [0]

    def on_vertex(level, rays, hits, records):
        if level == 0:
            shaded = (records.kind == KIND_SHADED) & records.has_next_ray
            total.add_(torch.where(shaded.unsqueeze(1), records.f * math.pi, torch.zeros_like(records.f)))
            samples[0] += 1

    film = integrator.render(scene, on_vertex=on_vertex).pixels
    mean = (total / max(samples[0], 1)).clamp(0.0, 1.0)
    albedo = torch.cat([mean, torch.ones_like(mean[:, :1])], dim=1).reshape(size, size, 4).cpu().numpy()
    return film, albedo


def main(argv):
    size = int(argv[1]) if len(argv) > 1 else 256
    spp = int(argv[2]) if len(argv) > 2 else 16
    out = argv[3] if len(argv) > 3 else "wavefront_path.png"
    out_albedo = argv[4] if len(argv) > 4 else "wavefront_albedo.png"
    pixels, albedo = render(size, spp)
    for name, px in ((out, pixels), (out_albedo, albedo)):
        film = pa.Film([size, size])
        film.pixels = px
        film.save(name)
        print(f"{name}: {size} x {size}, mean {float(px[..., :3].mean()):.4f}")


if __name__ == "__main__":
    main(sys.argv)
