"""``flygym_amd._handle`` without a GPU: the lifecycle of :class:`NativeHandle` against a stub library, the reset mask on a stub
simulation whose device is the CPU, and the params check of the seven structs against the built library's ``*_params_size()``."""

import ctypes
import gc

import numpy as np
import pytest
import torch

from flygym_amd import _native
from flygym_amd._handle import NativeHandle, check_params, reset_mask


class StubLib:
    def __init__(self, handle=1234, fail_destroy=False):
        self.handle, self.fail_destroy, self.destroyed, self.created_with = handle, fail_destroy, [], None

    def stub_create(self, *args):
        self.created_with = args
        return self.handle

    def stub_destroy(self, handle):
        self.destroyed.append(handle)
        if self.fail_destroy:
            raise OSError("destroy failed")

    def nmf_last_error(self):
        return b"stub_create: refused"


def make_thing(lib, **attrs):
    class Thing(NativeHandle):
        _destroy_entry, _noun, _views = "stub_destroy", "thing", ("a", "b")
        _lib = staticmethod(lambda: lib)

    for k, v in attrs.items():
        setattr(Thing, k, v)
    thing = Thing()
    thing.a, thing.b, thing.kept = "view a", ("view b0", "view b1"), "not a view"
    return thing


def test_close_destroys_once_and_clears_the_views():
    lib = StubLib()
    thing = make_thing(lib)
    assert thing._create("stub_create", 1, "x") == 1234 and lib.created_with == (1, "x")
    assert thing._h == 1234 and thing._handle() == 1234
    thing.close()
    assert thing._h is None and thing.a is None and thing.b is None and thing.kept == "not a view"
    with pytest.raises(RuntimeError, match="^the thing is closed$"):
        thing._handle()
    thing.close()
    del thing
    gc.collect()
    assert lib.destroyed == [1234]


def test_del_alone_destroys():
    lib = StubLib()
    thing = make_thing(lib)
    thing._create("stub_create")
    del thing
    gc.collect()
    assert lib.destroyed == [1234]


def test_with_closes():
    lib = StubLib()
    thing = make_thing(lib)
    thing._create("stub_create")
    with thing as inside:
        assert inside is thing and thing._handle() == 1234 and lib.destroyed == []
    assert lib.destroyed == [1234] and thing._h is None and thing.a is None
    with pytest.raises(RuntimeError, match="the thing is closed"):
        thing._handle()


def test_the_handle_attribute_is_the_subclass_s():
    lib = StubLib()
    thing = make_thing(lib, _handle_attr="_plan_h")
    thing._create("stub_create")
    assert thing._plan_h == 1234 and not hasattr(thing, "_h") and thing._handle() == 1234
    thing.close()
    assert thing._plan_h is None and lib.destroyed == [1234]


def test_an_exception_in_destroy_stays_inside_del():
    lib = StubLib(fail_destroy=True)
    thing = make_thing(lib)
    thing._create("stub_create")
    thing.__del__()                        # called directly: an exception would propagate to here
    assert lib.destroyed == [1234]
    with pytest.raises(OSError, match="destroy failed"):
        thing.close()                      # (close itself reports it)
    lib.fail_destroy = False
    thing.close()
    assert lib.destroyed == [1234] * 3 and thing._h is None


def test_a_null_creation_raises_native_error():
    lib = StubLib(handle=None)
    thing = make_thing(lib)
    with pytest.raises(_native.NativeError, match="^stub_create: refused$"):
        thing._create("stub_create")
    assert getattr(thing, "_h", None) is None
    with pytest.raises(RuntimeError, match="the thing is closed"):
        thing._handle()
    thing.close()
    del thing
    gc.collect()
    assert lib.destroyed == []


def test_a_subclass_chooses_the_creation_error():
    lib = StubLib(handle=0)
    thing = make_thing(lib, _creation_error=staticmethod(lambda msg: ValueError(msg) if "refused" in msg else KeyError(msg)))
    with pytest.raises(ValueError, match="stub_create: refused"):
        thing._create("stub_create")


class StubSim:
    _torch, device = torch, torch.device("cpu")


MASK = [1, 0, 0, 2, 0]


def test_no_mask_stays_none():
    assert reset_mask(None, 5, StubSim()) is None


@pytest.mark.parametrize("dtype", ["bool", "int32", "int64", "float32", "float64"])
@pytest.mark.parametrize("kind", ["numpy", "torch", "list"])
def test_masks_become_uint8(kind, dtype):
    mask = np.array(MASK).astype(dtype)
    mask = {"numpy": mask, "torch": torch.as_tensor(mask), "list": mask.tolist()}[kind]
    m = reset_mask(mask, 5, StubSim())
    assert m.dtype == torch.uint8 and tuple(m.shape) == (5,) and m.is_contiguous() and m.device == torch.device("cpu")
    assert m.tolist() == [1, 0, 0, 1, 0]


def test_a_strided_mask_becomes_contiguous():
    m = reset_mask(torch.as_tensor(np.array(MASK + MASK))[::2], 5, StubSim())
    assert m.is_contiguous() and m.tolist() == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("mask, got", [(np.zeros(4, dtype=bool), "(4,)"), (torch.zeros((5, 1)), "(5, 1)"), (True, "()")])
def test_a_mask_of_another_shape(mask, got):
    with pytest.raises(ValueError) as e:
        reset_mask(mask, 5, StubSim())
    assert str(e.value) == f"Expected a reset mask of shape (5,), but got {got}"


def the_seven():
    from flygym_amd.controllers import _CpgHybridParams, _CpgParams, _TaxisParams
    from flygym_amd.rendering import _CameraParams
    from flygym_amd.sensors import _OdometryParams, _PlumeParams
    from flygym_amd.vision import _EyeParams

    return [(_CpgParams, "nmf_cpg_params_size", "controllers.py"), (_CpgHybridParams, "nmf_cpg_hybrid_params_size", "controllers.py"),
            (_TaxisParams, "nmf_taxis_params_size", "controllers.py"), (_PlumeParams, "nmf_plume_params_size", "sensors.py"),
            (_OdometryParams, "nmf_odometry_params_size", "sensors.py"), (_EyeParams, "nmf_eye_params_size", "vision.py"),
            (_CameraParams, "nmf_camera_params_size", "rendering.py")]


@pytest.mark.parametrize("which", range(7))
def test_params_check_of_the_seven_structs(which):
    struct, size_entry, module_file = the_seven()[which]
    check_params(struct, size_entry, module_file)

    class Longer(ctypes.Structure):
        _fields_ = [("params", struct), ("one_more", ctypes.c_int32)]

    with pytest.raises(_native.NativeError) as e:
        check_params(Longer, size_entry, module_file)
    assert str(e.value) == f"{size_entry[:-5]} layout mismatch between {module_file} and libnmf_hip.so"
    assert size_entry[:-5].endswith("_params")
