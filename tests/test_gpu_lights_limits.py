"""The lights kernel (rtx_trace_lights) where tests/test_gpu_lights.py does not reach.

* A worker's second item at a cap above 0: the lanes of the second lap push and pop reflected rays (the lap
  test of tests/test_gpu_lights.py renders at cap 0, where nothing is pushed).
* The stack of 2B + 2 pending rays filled to its last entry, and overflowed by one: the kernel drops the ray
  and sets RTX_ST_STACK_OVERFLOW, the renderer raises RecursionError and the op RuntimeError. The kernel
  guards every push, so nothing is written out of bounds: the tests read an error channel.

The bar is tests/test_gpu_lights.py's: float64 colour within 1e-12 * max(1, |colour|) of the restatement with
an identical uint8 frame. tests/test_mesh_limits_cpu.py pins what each case exercises.
"""

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from python_ray_tracer_amd import lights, scenes, tiling
from tests import lights_ref as R
from tests.test_gpu_lights import RTOL, _check
from tests.test_mesh_limits_cpu import lap_case, lights_stack_case, second_lap_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from python_ray_tracer_amd.infrastructure import hip as H_

    return H_


def _op_args(r, scene, spec):
    """(blob, n_spheres, lights table, eye, directions) of ``scene``'s own frame for rt::trace_lights."""
    import python_ray_tracer_amd.ops  # noqa: F401

    blob, S = r.scene_blob(scene)
    table = torch.from_numpy(lights.lights_table(scene.lights)).cuda()
    dirs = r.get_ray_directions(scene.camera).data
    eye = torch.tensor([float(c) for c in spec["camera"]["position"]], dtype=torch.float64, device="cuda")
    return blob, S, table, eye, dirs


def test_a_frame_larger_than_the_pool_of_workers_at_cap_3(hip):
    """640 x 360 at cap 3: the workers of the frame's last rows take a second item and reflect there. Equal
    to the same frame in row tiles, none of which reaches a second lap, bit for bit; rows of both laps against
    the restatement; the uint8 and the float32 frame are the float64 frame's."""
    spec, cap, p, rows, want = lap_case("lights")
    W, H = spec["camera"]["width"], spec["camera"]["height"]
    scene = scenes.build_scene(spec)
    r = hip.HipRenderer(cap)
    flat = r.render(scene).data.cpu().numpy()
    full = flat.reshape(3, H, W)
    for part in range(4):
        tile_rows = tiling.tile_rows(H, 8, 4, part)
        assert W * len(tile_rows) < p
        tile = r.render_tile(scene, 8, 4, part).cpu().numpy()
        assert np.array_equal(tile, full[:, tile_rows].reshape(3, -1)), part
    _check(full[:, rows].reshape(3, -1), want, W, len(rows), f"rows {rows} of the 640x360 frame")
    lap2 = second_lap_rows("lights")
    _check(full[:, lap2].reshape(3, -1), want[:, -len(lap2) * W:], W, len(lap2), "the workers' second items")
    u8 = r.render_tile(scene, out="u8")
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), O.to_uint8(flat, W, H))
    got32 = hip.HipRenderer(cap, color_dtype=torch.float32).render(scene).data
    assert got32.dtype == torch.float32 and np.array_equal(got32.cpu().numpy(), flat.astype(np.float32))
    # a ray count that ends inside a wave of the second lap
    blob, S, table, eye, dirs = _op_args(r, scene, spec)
    n = p + 64 * 3 + 17
    assert p < n < dirs.shape[1]
    out = torch.ops.rt.trace_lights(blob, S, table, eye, dirs[:, :n].contiguous(), cap, 1)
    assert tuple(out.shape) == (3, n) and np.array_equal(out.cpu().numpy(), flat[:, :n])


def test_a_stack_filled_to_its_last_entry(hip):
    """Four coincident spheres at B = 1: 53 lit camera rays push 4 rays into 4 entries (the last push at
    sp == cap - 1), none needs more, nothing is reported."""
    spec, want, need = lights_stack_case(4)
    assert need.max() == 4 == 2 * 1 + 2
    got = hip.HipRenderer(1).render(scenes.build_scene(spec)).data.cpu().numpy()
    _check(got, want, 32, 18, "four coincident spheres")
    full = need == 4
    _check(got[:, full], want[:, full], int(full.sum()), 1, f"the {int(full.sum())} pixels with a full stack")


def test_an_overflowing_render_raises_every_time_and_leaves_nothing_behind(hip):
    """Five coincident spheres need 5 entries of 4, one more than the stack (a guard of sp <= cap would hold
    it, one entry past the end): RecursionError, again on the identical render (an overflowing key is not
    remembered as clean), and the same renderer, with the same workspace, then renders scenes that fit."""
    spec5, _, need5 = lights_stack_case(5)
    assert need5.max() == 5 == 2 * 1 + 2 + 1
    r = hip.HipRenderer(1)
    over = scenes.build_scene(spec5)
    for _ in range(2):
        with pytest.raises(RecursionError, match="maximum recursion depth exceeded.*more than 4 pending rays at max_bounces=1"):
            r.render(over)
    spec4, want4, _ = lights_stack_case(4)
    _check(r.render(scenes.build_scene(spec4)).data.cpu().numpy(), want4, 32, 18, "four coincident spheres after an overflow")
    plain = scenes.lights_spec(32, 18)
    _check(r.render(scenes.build_scene(plain)).data.cpu().numpy(), R.render(plain, 1), 32, 18, "lights_spec after an overflow")
    with pytest.raises(RecursionError, match="more than 4 pending rays at max_bounces=1"):  # and after clean renders
        r.render(over)


def test_an_overflow_through_the_op(hip):
    spec, want, need = lights_stack_case(5)
    scene = scenes.build_scene(spec)
    blob, S, table, eye, dirs = _op_args(hip.HipRenderer(1), scene, spec)
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        torch.ops.rt.trace_lights(blob, S, table, eye, dirs, 1, 1)
    with pytest.raises(RuntimeError, match="maximum recursion depth"):
        torch.ops.rt.trace_lights(blob, S, table, eye, dirs, 1, 1, check=True)
    got = torch.ops.rt.trace_lights(blob, S, table, eye, dirs, 1, 1, check=False).cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    fits = need <= 4
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    err = float(rel[:, fits].max())
    off = int((rel[:, ~fits] > RTOL).any(axis=0).sum())
    print(f"lanes that fit: max |gpu - ref| = {err:.3e}; {off} of the {int((~fits).sum())} overflowed lanes differ")
    assert int((~fits).sum()) == 53 and err <= RTOL  # only the overflowed lanes may differ
    assert off > 0  # (they dropped a ray)
