"""The host side's match of a model against the kernel families (``flygym_amd/csrc/nmf_skeleton.h`` over the family list of
``nmf_families.h``), run without a GPU: ``scripts/micro/classify_check.cpp`` is the blob parser and ``classify_skeleton`` with a
``main``, built under the address and undefined-behaviour sanitizers and run once over every blob below.

* the shipped presets and the custom skeletons land in the family the kernels were written for;
* near misses of a star family fall through to a general-tree family;
* what no kernel takes is refused with the message ``nmf_batch_create`` reports;
* the breadth-first tables are those of a plain walk of ``body_parent``.
"""

import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))


CUSTOM_TREE = ("ALL_BIOLOGICAL", ("wing", "haltere", "abdomen"))      # 105 dofs
CUSTOM_TREE_LARGE = ("ALL_POSSIBLE", ("wing", "haltere"))             # above the small tree family's 144 dofs


def _copy(model):
    out = type(model)({k: np.array(v) for k, v in model.items()})
    out.meta = dict(model.meta)
    return out


def _grow(model, count, n):
    """``model`` with the first rows of every per-actuator (``count="nu"``) or per-geom (``"ng"``) array repeated up to ``n``."""
    out, old = _copy(model), getattr(model, count)
    idx = np.arange(n) % old
    for k, v in model.items():
        if (k.startswith(("act_", "key_ctrl")) if count == "nu" else k.startswith(("geom_", "pair_"))) and v.ndim and v.shape[0] == old:
            out[k] = np.ascontiguousarray(v[idx])
    assert getattr(out, count) == n
    return out


def _edit(model, **arrays):
    out = _copy(model)
    for k, f in arrays.items():
        f(out[k])
    return out


def custom_world(preset, drop):
    """A world with the preset's skeleton without the joints of the named parts, leg actuators and adhesion: a general tree
    (``tests/test_hip_parity_r3.py::_fly("custom")``)."""
    import flygym_amd.compose as C
    from flygym_amd import anatomy as A
    from flygym_amd.utils.math import Rotation3D

    full = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=getattr(A.JointPreset, preset))
    keep = [j for j in full.anatomical_joints if not any(k in j.child.name for k in drop)]
    fly = C.Fly(name="t")
    fly.add_joints(A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, anatomical_joints=keep), neutral_pose=C.KinematicPosePreset.NEUTRAL)
    legs = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_actuators(legs.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_leg_adhesion()
    world = C.FlatGroundWorld()
    world.add_fly(fly, (0.3, 0.2, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return world


def _models():
    import tiny_models
    from flygym_amd import make_model

    m = {k: make_model(joints_preset=k)[1].compile_model() for k in ("legs_only", "legs_active_only", "all_biological", "all_possible")}
    m["sphere_on_plane"] = tiny_models.sphere_on_plane()
    m["hinge_on_heavy_base"] = tiny_models.hinge_on_heavy_base()
    m["welded_body"] = tiny_models.welded_body()
    m["custom_tree"] = custom_world(*CUSTOM_TREE).compile_model()
    m["custom_tree_large"] = custom_world(*CUSTOM_TREE_LARGE).compile_model()
    assert m["custom_tree"].nv <= 144 < m["custom_tree_large"].nv
    # near misses of a star family
    m["legs_only_49_actuators"] = _grow(m["legs_only"], "nu", 49)
    m["all_biological_65_actuators"] = _grow(m["all_biological"], "nu", 65)
    first_leg = m["all_biological"].nb - 6 * 8
    m["all_biological_leg_off_root"] = _edit(m["all_biological"], body_parent=lambda a: a.__setitem__(first_leg, 1))
    # what no kernel takes
    m["refuse_parent_after_child"] = _edit(m["custom_tree"], body_parent=lambda a: a.__setitem__(5, 7))
    m["refuse_geoms_unordered"] = _edit(m["custom_tree"], geom_body=lambda a: a.__setitem__(slice(None), a[::-1].copy()))
    m["refuse_deep"] = _edit(m["custom_tree"], body_parent=lambda a: a.__setitem__(slice(None), np.arange(-1, len(a) - 1)))
    m["refuse_129_geoms"] = _grow(m["legs_only"], "ng", 129)
    m["refuse_225_actuators"] = _grow(m["custom_tree"], "nu", 225)
    return m


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """(models, what the check program printed for each: a dict of its lines' first words to the rest)."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("classify")
    exe = tmp / "classify_check"
    # (plain C++ through hipcc: the sanitizers instrument the host program, there is no device code)
    flags = "-x c++ -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    res = subprocess.run(["hipcc", *flags.split(), f"-I{ROOT / 'flygym_amd' / 'csrc'}", str(ROOT / "scripts" / "micro" / "classify_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    models = _models()
    for name, model in models.items():
        (tmp / f"{name}.blob").write_bytes(model.to_blob())
    (tmp / "refuse_not_a_blob.blob").write_bytes(b"NMFMODEL")
    res = subprocess.run([str(exe), *[str(tmp / f"{n}.blob") for n in [*models, "refuse_not_a_blob"]]], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    out = {}
    for line in res.stdout.splitlines():
        if not line.startswith("  "):
            cur = out.setdefault(line[:-len(".blob")], {})
        else:
            key, _, rest = line.strip().partition(" ")
            cur[key] = rest
    return models, out


FAMILIES = {"legs_only": 0, "legs_active_only": 1, "all_biological": 4, "all_possible": 5,
            "sphere_on_plane": 2, "hinge_on_heavy_base": 2, "welded_body": 2, "custom_tree": 2, "custom_tree_large": 3,
            "legs_only_49_actuators": 2, "all_biological_65_actuators": 2, "all_biological_leg_off_root": 2}

REFUSALS = {"refuse_parent_after_child": "nmf_batch_create: bodies must be ordered parents first",
            "refuse_geoms_unordered": "nmf_batch_create: contact geoms must be ordered by body",
            "refuse_deep": "nmf_batch_create: kinematic tree deeper than 16 levels",
            "refuse_129_geoms": "nmf_batch_create: more than 128 contact geoms",
            "refuse_225_actuators": "nmf_batch_create: too many actuators (48 for the leg skeletons, 224 otherwise)",
            "refuse_not_a_blob": "nmf_model_create: not an NMFMODEL blob"}


@pytest.mark.parametrize("name", FAMILIES)
def test_family(checked, name):
    assert checked[1][name].get("family") == str(FAMILIES[name]), checked[1][name]


@pytest.mark.parametrize("name", REFUSALS)
def test_refusal_keeps_its_message(checked, name):
    assert checked[1][name] == {"refused": REFUSALS[name]}


def _breadth_first(parent, n_tree):
    """Bodies 0..n_tree-1 level by level, the children of a body contiguous: (level starts and the end, order, first child slot, children)."""
    order, lvl_start, child_start, child_count = [0], [0], [0] * len(parent), [0] * len(parent)
    while lvl_start[-1] < len(order):
        level = order[lvl_start[-1]:]
        lvl_start.append(len(order))
        for par in level:
            kids = [b for b in range(1, n_tree) if parent[b] == par]
            child_start[par], child_count[par] = len(order), len(kids)
            order += kids
    return lvl_start, order, child_start, child_count


@pytest.mark.parametrize("name", [n for n, f in FAMILIES.items() if f >= 2])
def test_tables_are_a_breadth_first_walk(checked, name):
    model, got = checked[0][name], checked[1][name]
    hybrid = FAMILIES[name] >= 4
    n_tree = model.nb - 6 * 8 if hybrid else model.nb      # hybrid families: the root and the rest of the body, legs left out
    want = _breadth_first(model["body_parent"].tolist(), n_tree)
    for key, w in zip(("lvl_start", "tree_body", "child_start", "child_count"), want):
        assert [int(x) for x in got[key].split()] == w, key
    if hybrid:      # the shipped full-body skeletons take the fast level passes: one pack entry per rest body
        pack = np.array(got["rest_pack"].split(), dtype=np.int64).reshape(-1, 2)
        assert got["rest_fast"] == "1" and sorted(pack[pack[:, 0] >= 0, 0] & 0xff) == list(range(1, n_tree))


@pytest.mark.parametrize("name", ["legs_only", "legs_active_only"])
def test_leg_chain_families_have_no_tables(checked, name):
    got = checked[1][name]
    assert got["lvl_start"] == got["tree_body"] == got["child_start"] == got["child_count"] == ""
