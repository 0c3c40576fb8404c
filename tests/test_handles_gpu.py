"""The six classes that own a handle of the library (``flygym_amd._handle.NativeHandle``) at their smallest legal shapes: one call of
the main method, ``close``, the views gone, the Python-level refusal afterwards, a silent second ``close``, the ``with`` form.
Nothing here passes a freed handle to the library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2


@pytest.fixture(scope="module")
def batch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flygym_amd import HIPSimulation, make_model

    fly, world, cam = make_model()                       # the flat ground
    sim = HIPSimulation(world, n_worlds=N, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((N, 6), dtype=np.float32))
    sim.reset()
    return torch, sim, fly, cam


def _turning(torch, sim, fly, cam):
    from flygym_amd.controllers import TurningCPG

    return TurningCPG(sim, fly.name, table_steps=1), lambda c: c.advance(1)


def _hybrid(torch, sim, fly, cam):
    from flygym_amd.controllers import HybridTurningCPG

    return HybridTurningCPG(sim, fly.name, table_steps=1), lambda c: c.advance(1)


def _plume(torch, sim, fly, cam):
    from flygym_amd.sensors import OdorPlume

    return OdorPlume(sim, fly.name, grid=(8, 8), cell_size=1.0, origin=(-4.0, -4.0), source=(0.0, 0.0, 1.0, 1.0)), lambda p: p.advance(1)


def _integrator(torch, sim, fly, cam):
    from flygym_amd.sensors import PathIntegrator

    return PathIntegrator(sim, fly.name, window=1), lambda o: o.update()


def _camera(torch, sim, fly, cam):
    from flygym_amd.rendering import HIPBatchRenderer

    out = torch.empty((1, 1, 8, 8, 3), dtype=torch.uint8, device=sim.device)
    return HIPBatchRenderer(sim, cam, camera_res=(8, 8), worlds=[0]), lambda r: r.render_into(out)


def _eyes(torch, sim, fly, cam):
    from flygym_amd.vision import EyeRenderer

    eyes = EyeRenderer(sim, fly.name)
    omm = torch.empty((N, 2, eyes.retina.num_ommatidia, 2), dtype=torch.float32, device=sim.device)
    return eyes, lambda e: e.render_into(omm)


CASES = {
    "TurningCPG": (_turning, "_h", ("phase", "magnitude", "drive")),
    "HybridTurningCPG": (_hybrid, "_h", ("phase", "magnitude", "drive", "retraction", "stumbling", "rule_flags")),
    "OdorPlume": (_plume, "_h", ("wind", "ticks", "buffers", "parity")),
    "PathIntegrator": (_integrator, "_h", ("stride_total", "window_strides", "heading", "position", "home", "count", "coefficients")),
    "HIPBatchRenderer": (_camera, "_plan_h", ()),
    "EyeRenderer": (_eyes, "_plan_h", ()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_use_close_refuse_and_with(batch, name):
    torch = batch[0]
    make, handle_attr, views = CASES[name]
    obj, use = make(*batch)
    assert type(obj).__name__ == name and tuple(obj._views) == views and obj._handle_attr == handle_attr
    assert getattr(obj, handle_attr) and all(getattr(obj, v) is not None for v in views)
    use(obj)
    torch.cuda.synchronize()
    obj.close()
    assert getattr(obj, handle_attr) is None
    for v in views:
        assert getattr(obj, v) is None, v
    with pytest.raises(RuntimeError, match="closed"):
        use(obj)
    obj.close()                                          # silent

    second, use = make(*batch)
    with second as inside:
        assert inside is second
        use(second)
        torch.cuda.synchronize()
    assert getattr(second, handle_attr) is None and all(getattr(second, v) is None for v in views)
    with pytest.raises(RuntimeError, match="closed"):
        use(second)
