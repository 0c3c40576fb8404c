"""Every kernel family of ``flygym_amd/csrc/nmf_families.h`` on the GPU: a model of each lands on its family's kernel, with
the contact-space flavour, contact capacity and chunk plan its topology type implies, and steps.

The expected rows were read off ``batch_info()`` of the commit before the host side asked the types (family numbers, control
caps and patterns spelt out by hand in ``nmf_capi.hip``), one run, these models."""

import numpy as np
import pytest

from test_classify_check import CUSTOM_TREE, CUSTOM_TREE_LARGE, custom_world

pytestmark = pytest.mark.gpu

# model -> kernel_family, contact_space_flavour, contact_space_max_contacts, chunk_div_x1000
EXPECTED = {"legs_only": (0, 1, 16, 1700), "legs_active_only": (1, 1, 16, 1700), "custom_tree": (2, 0, 0, 2000),
            "custom_tree_large": (3, 0, 0, 2000), "all_biological": (4, 2, 13, 2000), "all_possible": (5, 2, 13, 2000)}


def _world(name):
    from flygym_amd import make_model

    if name.startswith("custom"):
        return custom_world(*(CUSTOM_TREE_LARGE if name == "custom_tree_large" else CUSTOM_TREE))
    return make_model(joints_preset=name)[1]


@pytest.mark.parametrize("name", EXPECTED)
def test_family_of_a_batch_and_one_step(name):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flygym_amd import HIPSimulation

    sim = HIPSimulation(_world(name), n_worlds=2, device=0)
    info = sim.batch_info()
    got = tuple(info[k] for k in ("kernel_family", "contact_space_flavour", "contact_space_max_contacts", "chunk_div_x1000"))
    print(name, got, {k: info[k] for k in ("flies_per_cu", "resident_workgroups", "chunked")})
    assert got == EXPECTED[name]
    sim.step(1)
    torch.cuda.synchronize()
    assert np.isfinite(sim.field("qpos").cpu().numpy()).all()
