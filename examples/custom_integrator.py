#!/usr/bin/env python3
"""examples/custom_integrator.py -- a CustomRayIntegrator (core/integrator.h:61-74) written in torch over Accel's ray queries.

The reference lets a script supply radiance(ray) and gives it intersect(ray, it) and hit(ray); here the same two questions are
asked for whole batches on the GPU, and the integrator between them is ordinary torch code on device tensors:

    camera rays -> accel.intersect -> for the hits, one shadow ray to a point light -> accel.hit -> N.L, no albedo -> PNG

    python examples/custom_integrator.py [size] [out.png] [pine|embree]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import pine_amd as pa  # noqa: E402
from pine_amd import scenes  # noqa: E402

LIGHT = (0.0, 1.8, 1.0)  # a point light under the Cornell box's lamp


def radiance(accel, rays, light):
    """(N, 3) radiance of N rays: the cosine between the surface normal and the direction to `light` where the light is
    visible from the hit, 0 elsewhere (misses included)."""
    it = accel.intersect(rays)
    hit = it.geometry >= 0
    n = torch.where((it.n * rays[:, 3:6]).sum(1, keepdim=True) > 0, -it.n, it.n)  # (turned towards the viewer)
    to_light = torch.tensor(light, dtype=torch.float32, device=rays.device) - it.p
    dist = to_light.norm(dim=1, keepdim=True).clamp_min(1e-12)
    wi = to_light / dist
    shadow = torch.zeros_like(rays)
    shadow[:, 0:3] = it.p + 1e-3 * n  # (off the surface)
    shadow[:, 3:6] = wi               # (unit length: t is a distance)
    shadow[:, 7] = (dist[:, 0] - 2e-3).clamp_min(0.0)
    visible = accel.hit(shadow) == 0
    cos = (n * wi).sum(1).clamp_min(0.0)
    return (cos * (hit & visible)).unsqueeze(1).expand(-1, 3)


def render(size=64, order="pine", device=0):
    """The (size, size, 4) film of the Cornell box under the custom integrator, a numpy array."""
    scene = scenes.cbox((size, size), "readme")
    with pa.Accel(scene, order=order, device=device) as accel:
        rays = accel.camera_rays(tensor=True)
        L = radiance(accel, rays, LIGHT)
        film = torch.cat([L, torch.ones_like(L[:, :1])], dim=1).reshape(size, size, 4)
        return film.cpu().numpy()


def main(argv):
    size = int(argv[1]) if len(argv) > 1 else 256
    out = argv[2] if len(argv) > 2 else "custom_integrator.png"
    order = argv[3] if len(argv) > 3 else "pine"
    film = pa.Film([size, size])
    film.pixels = render(size, order)
    film.save(out)
    print(f"{out}: {size} x {size}, mean {float(film.pixels[..., :3].mean()):.4f}")


if __name__ == "__main__":
    main(sys.argv)
