"""CPU: the denoising filter of pine_amd/csrc/pine_denoise.h through its host-thread build (device=-1) -- against an independent
float64 numpy restatement of its definition, its structure (identity, misses, alpha, small and ragged films, thread count) and
the one thing it is for: on every fixture scene the filtered noisy film is closer to the converged film than the noisy one is.

Tolerance of the restatement comparison.  The host build rounds every operation to fp32, the restatement computes in float64
from the same fp32 inputs; the difference is rounding, and it differs per input.  Measured on this suite's four fixtures with
default parameters: the largest absolute difference of any output component is 7.765e-06 (cbox_readme_64; its outputs reach
225), so the tests allow RESTATEMENT_TOL = 4 x that = 3.106e-05.  The same numbers, and the effect of mutations of the
restatement, are in profiles/denoise_quality.txt (tools/denoise_quality.py writes it): one tap dropped, one offset mirrored or
step i instead of 2^i move the difference to at least 5.7e-03 = 184 x the tolerance on every fixture; skipping the hit(q) gate
moves nothing, because a miss's zero normal already gives the tap the weight 0 -- the gate matters only when a miss's
demodulated colour overflows fp32 (test_misses_contribute_nothing_whatever_their_colour)."""
import os
import subprocess

import numpy as np
import pytest

import denoise_scenes as S

F32 = np.float32
RESTATEMENT_MEASURED = 7.765e-06
RESTATEMENT_TOL = 4 * RESTATEMENT_MEASURED
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def defaults():
    from pine_amd import api
    p = api.denoise_params()
    return dict(iterations=p.iterations, normal_power_log2=p.normal_power_log2, sigma_color=float(F32(p.sigma_color)),
                sigma_albedo=float(F32(p.sigma_albedo)), eps_albedo=float(F32(p.eps_albedo)))


def restate(film, albedo, normal, iterations, normal_power_log2, sigma_color, sigma_albedo, eps_albedo, mutate=None):
    """The filter's definition (pine_amd/csrc/pine_denoise.h) in float64, vectorised over the film, one tap at a time.
    mutate: None, or one of "drop_tap", "mirror_offset", "no_hit_gate", "linear_step" (tools/denoise_quality.py)."""
    F = film.astype(np.float64)
    A = albedo.astype(np.float64)
    N = normal.astype(np.float64)
    h, w = F.shape[:2]
    if iterations == 0:
        return F.copy()
    hit = (normal != 0).any(axis=2)
    D = np.maximum(A, np.float64(F32(eps_albedo)))
    I = F[..., :3] / D
    ys, xs = np.mgrid[0:h, 0:w]
    sa2 = np.float64(F32(sigma_albedo)) ** 2
    for i in range(iterations):
        s = i if mutate == "linear_step" else 2 ** i
        sc2 = (np.float64(F32(sigma_color)) * 2.0 ** -i) ** 2
        num = np.zeros((h, w, 3))
        den = np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if mutate == "drop_tap" and (dx, dy) == (1, -1):
                    continue
                ox = -dx if mutate == "mirror_offset" and (dx, dy) == (1, 0) else dx
                qy, qx = ys + s * dy, xs + s * ox
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                ok = inside & (hit[qy, qx] if mutate != "no_hit_gate" else True)
                Iq = I[qy, qx]
                if dx == 0 and dy == 0:
                    wgt = np.ones((h, w))
                else:
                    wn = np.maximum(0.0, (N * N[qy, qx]).sum(axis=2)) ** (2 ** normal_power_log2)
                    wa = np.exp(-((A - A[qy, qx]) ** 2).sum(axis=2) / sa2)
                    wc = np.exp(-((I - Iq) ** 2).sum(axis=2) / sc2)
                    wgt = wn * wa * wc
                c = np.where(ok, H5[dx + 2] * H5[dy + 2] * wgt, 0.0)
                num += c[..., None] * Iq
                den += c
        I = np.where(hit[..., None], num / np.where(den > 0, den, 1.0)[..., None], I)
    out = F.copy()
    out[..., :3] = np.where(hit[..., None], I * D, F[..., :3])
    return out


def host(film, albedo, normal, **params):
    import pine_amd as pa
    return pa.denoise(film, albedo, normal, device=-1, **params)


@pytest.fixture(scope="module")
def fixtures():
    return {name: S.load(name) for name in S.DENOISE_FILMS}


@pytest.fixture(scope="module")
def denoised(fixtures):
    """The noisy film of every fixture through the host build, default parameters: computed once, left unchanged."""
    return {name: host(f["noisy"], f["albedo"], f["normal"]) for name, f in fixtures.items()}


@pytest.mark.parametrize("name", list(S.DENOISE_FILMS))
def test_host_build_equals_float64_restatement(name, fixtures, denoised):
    f = fixtures[name]
    want = restate(f["noisy"], f["albedo"], f["normal"], **defaults())
    diff = np.abs(denoised[name].astype(np.float64) - want).max()
    print(f"{name}: max |host - restatement| = {diff:.3e} (tolerance {RESTATEMENT_TOL:.3e})")
    assert np.isfinite(denoised[name]).all()
    assert diff <= RESTATEMENT_TOL


@pytest.mark.parametrize("name", list(S.DENOISE_FILMS))
def test_denoised_is_closer_to_converged(name, fixtures, denoised):
    f = fixtures[name]
    hit = S.hits(f["normal"])
    conv = f["converged"][..., :3].astype(np.float64)[hit]
    before = ((f["noisy"][..., :3].astype(np.float64)[hit] - conv) ** 2).mean()
    after = ((denoised[name][..., :3].astype(np.float64)[hit] - conv) ** 2).mean()
    print(f"{name}: mse noisy {before:.5g}, denoised {after:.5g}, ratio {after / before:.4f}")
    assert after < before


def test_zero_iterations_is_the_identity(fixtures):
    f = fixtures["xshapes_48"]
    out = host(f["noisy"], f["albedo"], f["normal"], iterations=0)
    assert np.array_equal(out.view(np.uint32), f["noisy"].view(np.uint32))


@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_misses_and_alpha_are_unchanged(iterations, fixtures):
    f = fixtures["xshapes_48"]
    film = f["noisy"].copy()
    film[..., 3] = np.linspace(0.25, 4.0, film[..., 3].size, dtype=F32).reshape(film.shape[:2])
    out = host(film, f["albedo"], f["normal"], iterations=iterations)
    miss = ~S.hits(f["normal"])
    assert miss.mean() >= 0.01
    assert np.array_equal(out[miss].view(np.uint32), film[miss].view(np.uint32))
    assert np.array_equal(out[..., 3].view(np.uint32), film[..., 3].view(np.uint32))
    assert not np.array_equal(out[~miss][:, :3], film[~miss][:, :3])


def test_misses_contribute_nothing_whatever_their_colour(fixtures):
    """A miss's colour over eps_albedo overflows fp32 here: were a miss read at all, 0 x inf would poison its neighbours."""
    f = fixtures["xshapes_48"]
    miss = ~S.hits(f["normal"])
    film = f["noisy"].copy()
    film[miss, :3] = 3e38
    out = host(film, f["albedo"], f["normal"])
    want = host(f["noisy"], f["albedo"], f["normal"])
    assert np.isfinite(out).all()
    assert np.array_equal(out[~miss].view(np.uint32), want[~miss].view(np.uint32))
    assert np.array_equal(out[miss].view(np.uint32), film[miss].view(np.uint32))


def test_a_film_that_is_a_multiple_of_the_albedo_comes_back(fixtures):
    """F = c A on hits: the demodulated colour is constant, every weighted mean of it is that constant."""
    f = fixtures["mats_zoo_64"]
    hit = S.hits(f["normal"])
    film = np.zeros(f["noisy"].shape, F32)
    film[..., :3] = F32(2.5) * np.maximum(f["albedo"], F32(defaults()["eps_albedo"]))
    film[..., 3] = 1
    film[~hit, :3] = 0.125
    out = host(film, f["albedo"], f["normal"])
    assert np.abs(out.astype(np.float64) - film).max() <= RESTATEMENT_TOL
    assert np.array_equal(out[~hit], film[~hit])


def random_case(w, h, seed, misses=True):
    rng = np.random.default_rng(seed)
    film = (rng.random((h, w, 4)) * 3).astype(F32)
    albedo = (rng.random((h, w, 3)) * 0.9).astype(F32)
    albedo[rng.random((h, w)) < 0.1] = 0  # (black albedos: demodulation by eps_albedo)
    n = rng.normal(size=(h, w, 3))
    n[rng.random((h, w)) < 0.5] = [0.0, 0.0, -1.0]  # (half the film one flat wall: normal weights of 1)
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F32)
    if misses:
        miss = rng.random((h, w)) < 0.15
        normal[miss] = 0
        albedo[miss] = 0
    return film, albedo, normal


SMALL_FILMS = [(1, 1), (3, 2), (20, 12), (45, 37)]  # one pixel | less than one tap ring | less than the last step's reach | ragged


@pytest.mark.parametrize("size", SMALL_FILMS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_small_and_ragged_films(size, iterations):
    film, albedo, normal = random_case(size[0], size[1], 7 + size[0], misses=size != (1, 1))
    prm = dict(defaults(), iterations=iterations)
    out = host(film, albedo, normal, iterations=iterations)
    want = restate(film, albedo, normal, **prm)
    assert out.shape == film.shape and np.isfinite(out).all()
    assert np.abs(out.astype(np.float64) - want).max() <= RESTATEMENT_TOL
    if size == (1, 1):  # (the centre tap alone: the pixel's own colour, demodulated and back)
        assert np.abs(out.astype(np.float64) - film).max() <= 1e-6


def test_output_is_independent_of_the_host_thread_count(monkeypatch, fixtures):
    f = fixtures["cbox_readme_64"]
    outs = []
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("OMP_NUM_THREADS", threads)
        outs.append(host(f["noisy"], f["albedo"], f["normal"]))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))


def test_bad_parameters_are_refused():
    import pine_amd as pa
    film, albedo, normal = random_case(4, 4, 1)
    for bad in (dict(iterations=-1), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_albedo=-1.0), dict(normal_power_log2=40)):
        with pytest.raises(pa.PineError, match="denoise"):
            host(film, albedo, normal, **bad)
    with pytest.raises(pa.PineError, match="unknown parameter"):
        host(film, albedo, normal, radius=3)
    with pytest.raises(pa.PineError, match=r"\(H, W, 4\)"):
        host(film[..., :3], albedo, normal)


def test_defaults_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(S.GOLDEN)), "include", "pine_gpu.h")).read()
    d = defaults()
    assert d["iterations"] == 5 and d["normal_power_log2"] == 7
    for key, macro in (("sigma_color", "SIGMA_COLOR"), ("sigma_albedo", "SIGMA_ALBEDO"), ("eps_albedo", "EPS_ALBEDO")):
        line = [ln for ln in text.splitlines() if ln.startswith(f"#define PINE_GPU_DENOISE_{macro} ")][0]
        assert float(F32(float(line.split()[2].rstrip("f")))) == d[key]


def test_guides_and_the_device_filter_need_a_gpu():
    """No CPU path behind the guide pass, and device >= 0 means the device: without one both raise."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pine_amd as pa
    scene = S.denoise_scene("cbox_8x1")
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.guides(scene)
    film, albedo, normal = random_case(4, 4, 1)
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.denoise(film, albedo, normal, device=0)
    with pytest.raises(pa.PineError):
        pa.DenoiseIntegrator().render(scene)


def test_prl_has_no_denoise():
    """In the reference as built denoise(scene) leaves every colour unchanged; a script must keep rendering what the reference
    renders, so the language does not know the filter: it is the command line's --denoise."""
    from pine_amd import prl
    with pytest.raises(prl.PrlError):
        prl.interpret("s := Scene(); denoise(s);", dry_run=True)


def test_cpp_facade_example_compiles(tmp_path):
    root = os.path.dirname(os.path.dirname(S.GOLDEN))
    lib_dir = os.path.join(root, "pine_amd", "lib")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(root, "examples", "denoise.cpp"), "-L" + lib_dir, "-lpine_gpu",
                        "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "denoise_cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
