"""The glass kernel (rtx_trace_glass) where tests/test_gpu_glass.py does not reach.

* A worker's second item: the kernel runs a bounded pool of workers, each looping over ray items with
  one stack of pending rays; frames and ray sets larger than the pool (taken from the library, never
  from a constant here) put glass into the second lap.
* The stack of 4B + 4 pending rays filled to its last entry, and overflowed: the kernel drops the ray
  and sets RTX_ST_STACK_OVERFLOW, the renderer raises RecursionError and the op RuntimeError. The
  kernel guards every push, so nothing is written out of bounds: the tests read an error channel.
* The ends of the cap range ride on CASES (cap0, cap1, cap7, cap8; test_frames_against_the_restatement).
* Rays grazing a glass ball, where the exit's max(1 - ior^2 (1 - ce^2), 0) is taken.

The bars are test_gpu_glass.py's: float64 colour within ATOL = 1e-12 of the restatement with an
identical uint8 frame, and at least half of the restatement's changed pixels differing from the
opaque frame. tests/test_glass_cpu.py pins what each case sends where.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import scenes
from tests import glass_ref as G
from tests.test_glass_cpu import GRAZING, LAPS, _changed_mask, frame, grazing_case, lap_frame, stack_case
from tests.test_gpu_glass import ATOL, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _vec(hip, a):
    """Three rows of a host array as a device HipVector3D."""
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(a))).cuda()
    return hip.HipVector3D(dev[0], dev[1], dev[2])


def _op_args(r, scene, spec):
    """(blob, n_spheres, side table, eye, directions) of ``scene``'s own frame for rt::trace_glass."""
    import python_ray_tracer_amd.ops  # noqa: F401
    from python_ray_tracer_amd import glass

    blob, S = r.scene_blob(scene)
    table = torch.from_numpy(glass.glass_table(scene.shapes)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    return blob, S, table, eye, dirs


# ---- the stack at its capacity and over it -------------------------------------------------------------------

def test_a_stack_filled_to_its_last_entry(hip):
    """Four coincident spheres at B = 1: 53 lit camera rays push 8 rays into 8 entries (the push at
    sp == cap - 1), none needs more, nothing is reported."""
    spec, gains, want, counts, plain, need = stack_case(4)
    assert need.max() == 8 == 4 * 1 + 4
    got = hip.HipRenderer(1).render(scenes.build_scene(G.with_gains(spec, gains))).data.cpu().numpy()
    _check(got, want, 32, 18, "four coincident spheres")
    full = need == 8
    _check(got[:, full], want[:, full], int(full.sum()), 1, "the 53 pixels with a full stack")
    moved, changed = int(_changed_mask(got, plain, 32, 18).sum()), int(_changed_mask(want, plain, 32, 18).sum())
    print(f"{moved} uint8 pixels differ from the opaque frame ({changed} in the restatement)")
    assert moved >= (changed + 1) // 2 > 0


def test_an_overflowing_render_raises_every_time_and_leaves_nothing_behind(hip):
    """Five coincident spheres need 10 entries of 8: RecursionError, again on the identical render (an
    overflowing key is not remembered as clean), and the same renderer, with the same workspace, then
    renders scenes that fit: the sticky flag was cleared and the stacks hold nothing that matters."""
    spec5, gains5, _, _, _, need5 = stack_case(5)
    assert need5.max() == 10 > 8
    r = hip.HipRenderer(1)
    over = scenes.build_scene(G.with_gains(spec5, gains5))
    for _ in range(2):
        with pytest.raises(RecursionError, match="maximum recursion depth exceeded.*8 pending rays at max_bounces=1"):
            r.render(over)
    spec4, gains4, want4 = stack_case(4)[:3]
    _check(r.render(scenes.build_scene(G.with_gains(spec4, gains4))).data.cpu().numpy(), want4, 32, 18,
           "four coincident spheres after an overflow")
    readme, gains = scenes.readme_spec(32, 18), [0.9, 0.9, 0.0]
    _check(r.render(scenes.build_scene(G.with_gains(readme, gains))).data.cpu().numpy(), G.render(readme, gains, None, 1),
           32, 18, "the README scene after an overflow")
    with pytest.raises(RecursionError):  # and an overflow after clean renders is still seen
        r.render(over)


def test_an_overflow_by_one_entry(hip):
    """Five coincident spheres of which the last sends no reflected ray: 9 pending rays, one more than
    the stack holds. It must be reported (a guard of sp <= cap would hold it, one entry past the end)."""
    spec, gains, _, _, _, need = stack_case(5, 1)
    assert need.max() == 9 == 4 * 1 + 4 + 1
    with pytest.raises(RecursionError, match="maximum recursion depth exceeded"):
        hip.HipRenderer(1).render(scenes.build_scene(G.with_gains(spec, gains)))


@pytest.mark.parametrize("matt", [0, 1])
def test_an_overflow_through_the_op(hip, matt):
    spec, gains, want, _, _, need = stack_case(5, matt)
    scene = scenes.build_scene(G.with_gains(spec, gains))
    blob, S, table, eye, dirs = _op_args(hip.HipRenderer(1), scene, spec)
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        torch.ops.rt.trace_glass(blob, S, table, eye, dirs, 1, 1)
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        torch.ops.rt.trace_glass(blob, S, table, eye, dirs, 1, 1, check=True)
    got = torch.ops.rt.trace_glass(blob, S, table, eye, dirs, 1, 1, check=False).cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    fits = need <= 8
    assert int(fits.sum()) == 32 * 18 - 53
    err = float(np.abs(got - want)[:, fits].max())
    off = int((np.abs(got - want) > ATOL).any(axis=0).sum())
    print(f"lanes that fit: max |gpu - ref| = {err:.3e}; {off} of the 53 overflowed lanes differ")
    assert err <= ATOL  # only the overflowed lanes may differ
    assert off > 0  # (they dropped rays)


def test_cap_zero_is_the_opaque_frame(hip):
    spec, gains, cap, want, _, _ = frame("cap0")
    got = hip.HipRenderer(0).render(scenes.build_scene(G.with_gains(spec, gains))).data.cpu().numpy()
    _check(got, O.render(O.scene_from_spec(spec), 0), 32, 18, "cap 0 against the oracle's opaque frame")


# ---- frames and ray sets larger than the pool of workers -----------------------------------------------------

@pytest.mark.parametrize("key", sorted(LAPS))
def test_frames_larger_than_the_pool(hip, key):
    spec, gains, cap, want, plain, p = lap_frame(key)
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    n = W * H
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(cap)
    got = r.render(scene).data.cpu().numpy()
    _check(got, want, W, H, key)
    _check(got[:, :p], want[:, :p], p, 1, f"{key}, the workers' first items")
    _check(got[:, p:], want[:, p:], n - p, 1, f"{key}, the workers' second items")
    moved = int(_changed_mask(got, plain, W, H)[p:].sum())
    print(f"{key}: {moved} uint8 pixels of the second lap differ from the opaque frame ({LAPS[key][3]} in the restatement)")
    assert moved >= (LAPS[key][3] + 1) // 2
    u8 = r.render_tile(scene, out="u8")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
    assert np.array_equal(u8.cpu().numpy(), O.to_uint8(want, W, H))
    if cap == 3:
        got32 = hip.HipRenderer(cap, color_dtype=torch.float32).render(scene).data
        assert got32.dtype == torch.float32
        assert np.array_equal(got32.cpu().numpy(), got.astype(np.float32))  # the float64 value rounded once


def test_explicit_rays_with_per_ray_origins_larger_than_the_pool(hip):
    """test_explicit_rays_with_per_ray_origins on the B = 8 frame's rays: one origin per ray
    (org_stride = n) read at i >= n_workers."""
    spec, gains, cap, _, _, p = lap_frame("lap_B8")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    osc, g, iors = G.scene_of(spec, gains)
    cam = tuple(float(c) for c in osc.cam)
    d = np.stack(O.ray_directions(osc.cam, W, H))
    n = d.shape[1]
    back = np.linspace(0.0, 0.5, n)
    o = np.stack([cam[c] - d[c] * back for c in range(3)])
    want = np.stack(G.trace(osc, g, iors, tuple(o), tuple(d), cap))
    scene = scenes.build_scene(G.with_gains(spec, gains))
    got = hip.HipRenderer(cap).raytrace_scene(_vec(hip, o), _vec(hip, d), scene).data.cpu().numpy()
    _check(got, want, W, H, "per-ray origins")
    _check(got[:, p:], want[:, p:], n - p, 1, "per-ray origins, the workers' second items")
    plain = np.stack(O.trace(O.scene_from_spec(spec), tuple(o), tuple(d), cap))
    assert int(_changed_mask(got, plain, W, H)[p:].sum()) >= 4777  # (9,554 measured in the restatement)


def test_a_ray_count_that_ends_inside_a_wave_of_the_second_lap(hip):
    spec, gains, cap, want, _, p = lap_frame("lap_B3")
    scene = scenes.build_scene(G.with_gains(spec, gains))
    r = hip.HipRenderer(cap)
    full = r.render(scene).data
    blob, S, table, eye, dirs = _op_args(r, scene, spec)
    n = p + 64 * 3 + 17
    assert p < n < dirs.shape[1]
    out = torch.ops.rt.trace_glass(blob, S, table, eye, dirs[:, :n].contiguous(), cap, 1)
    assert tuple(out.shape) == (3, n) and torch.equal(out, full[:, :n])
    _check(out.cpu().numpy(), want[:, :n], n, 1, f"the first {n} rays")


# ---- grazing rays and the exit clamp -------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(GRAZING), ids=lambda c: f"sphere{c[0]}-ior{c[1]}")
def test_grazing_rays(hip, case):
    """200,000 parallel rays past the limb of a glass ball (impact parameter r (1 - eps), eps from 1e-16
    to 1e-6): c < 0, the correctly rounded divide and square root and the exit's clamp decide bit for bit
    like the restatement, or a ray goes elsewhere and its colour moves by far more than ATOL."""
    si, ior = case
    spec, gains, iors, o, d, want, counts = grazing_case(si, ior)
    assert counts.clamps == GRAZING[case] > 0
    n = want.shape[1]
    scene = scenes.build_scene(spec)
    got = hip.HipRenderer(2).raytrace_scene(_vec(hip, o), _vec(hip, d), scene).data.cpu().numpy()
    _check(got, want, n, 1, f"sphere {si}, ior {ior} ({counts.clamps} clamped exits)")
    plain = np.stack(G.trace(G.scene_of(spec, gains, iors)[0], [0.0] * 3, iors, o, d, 2))  # the same indices, opaque
    assert int(_changed_mask(got, plain, n, 1).sum()) >= 41000  # (82,415 to 89,041 measured in the restatement)
