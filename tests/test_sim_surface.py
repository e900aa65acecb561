"""The public surface of adaptigraph_amd.sim, frozen where the package replaced the single module; SimEnv without private reach-in; the datasets
of adaptigraph_amd.datagen against digests recorded before its loops were merged (tests/golden/datagen_digests.json, tools/gen_datagen_digests.py)."""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest

from adaptigraph_amd import configs, sim, sim_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every top-level name of sim.py without a leading underscore, as the single module had them (its imports included)
PUBLIC = ['dataclasses', 'math', 'np', 'MAX_PARTICLES', 'F32', 'SimParams', 'DEFAULT', 'stiffness_mapping', 'RopeScene', 'push_steps', 'frames_of',
          'rope_push_host', 'rope_push_scalar', 'DevicePush', 'rope_push', 'initial_rope', 'sample_push', 'PILE_MAX_PARTICLES', 'PILE_RHO_MAX',
          'PILE_KEY_OFFSETS', 'PileParams', 'PILE_DEFAULT', 'PileScene', 'board_lateral', 'pile_push_host', 'pile_push_scalar', 'DevicePilePush',
          'pile_push', 'initial_pile', 'board_clearance', 'sample_board_push', 'CLOTH_MAX_PARTICLES', 'CLOTH_MAX_SIDE', 'CLOTH_PICK_K', 'ClothParams',
          'CLOTH_DEFAULT', 'cloth_stiffness_mapping', 'ClothScene', 'cloth_phases', 'grasp_steps', 'cloth_pick', 'cloth_push_host',
          'cloth_push_scalar', 'DeviceClothPush', 'cloth_push', 'initial_cloth', 'cloth_border', 'sample_grasp', 'BOX_MAX_PARTICLES', 'BOX_SIDE_MAX',
          'BOX_RHO_MAX', 'BOX_K_MAX', 'BOX_COM_MAX', 'BoxParams', 'BOX_DEFAULT', 'box_masses', 'box_particles', 'BoxScene', 'box_push_host',
          'box_push_scalar', 'DeviceBoxPush', 'box_push', 'initial_box', 'sample_box_push']

ROPE = "SimParams(dt=0.016666666666666666, substeps=8, g=9.8, r=0.03, R=0.05, mu=0.1, speed=0.01, record_every=10, settle=120, lift=0.2)"
PILE = ("PileParams(dt=0.016666666666666666, substeps=8, iters=4, g=9.8, mu=1.0, W=0.5, T=0.02, slack=1.9073486328125e-06, tool_y=0.1, speed=0.01, "
        "record_every=10, settle=120, lift=0.2)")
CLOTH = ("ClothParams(dt=0.016666666666666666, substeps=4, iters=4, g=9.8, r=0.03, drag=1.0, speed=0.02, lift=0.5, grasp=0.1, finger=0.2, "
         "tool_y=0.03, record_every=5, settle=120)")
BOX = ("BoxParams(dt=0.016666666666666666, substeps=8, iters=2, g=9.8, mu=0.5, r=0.04, R=0.1, eps=0.001, v_rest=0.001, depen=2.0, speed=0.01, "
       "record_every=10, settle=30, lift=0.2)")
SIGNATURES = {
    "rope_push": f"(scene, push, params={ROPE}, f_max=None, device='cuda:0')",
    "pile_push": f"(scene, push, params={PILE}, f_max=None, device='cuda:0')",
    "cloth_push": f"(scene, action, params={CLOTH}, f_max=None, device='cuda:0')",
    "box_push": f"(scene, push, params={BOX}, f_max=None, device='cuda:0')",
    "rope_push_host": f"(scene, push, params={ROPE}, f_max=None)",
    "pile_push_host": f"(scene, push, params={PILE}, f_max=None, trace=None)",
    "cloth_push_host": f"(scene, action, params={CLOTH}, f_max=None)",
    "box_push_host": f"(scene, push, params={BOX}, f_max=None)",
    "DevicePush.__init__": f"(self, scene, push, params={ROPE}, f_max=None, device='cuda:0')",
    "DevicePilePush.__init__": f"(self, scene, push, params={PILE}, f_max=None, device='cuda:0', rho_max=None)",
    "DeviceClothPush.__init__": f"(self, scene, action, params={CLOTH}, f_max=None, device='cuda:0')",
    "DeviceBoxPush.__init__": f"(self, scene, push, params={BOX}, f_max=None, device='cuda:0')",
}


def test_public_names():
    assert [n for n in PUBLIC if not hasattr(sim, n)] == []


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures(name):
    obj = sim
    for part in name.split("."):
        obj = getattr(obj, part)
    assert str(inspect.signature(obj)) == SIGNATURES[name]


def _code_names(code):
    """Every name a code object and the code objects nested in it refer to."""
    names = set(code.co_names)
    for const in code.co_consts:
        if inspect.iscode(const):
            names |= _code_names(const)
    return names


def test_sim_env_uses_no_private_name_of_sim():
    with open(sim_env.__file__) as f:
        names = _code_names(compile(f.read(), sim_env.__file__, "exec"))
    private = {n for pkg in (sim, sim._common, sim.rope, sim.pile, sim.cloth, sim.box) for n in vars(pkg) if n.startswith("_") and not n.startswith("__")}
    assert "_validate" in private and "_box_validate" in private          # (the set is not empty for a trivial reason)
    assert sorted(names & private) == []
    assert [n for n in names if n.startswith("_") and not n.startswith("__") and hasattr(sim, n)] == []


def _scene(material):
    rng = np.random.default_rng(5)
    if material == "rope":
        return sim.RopeScene.from_ropes([sim.initial_rope(rng, 10)], stiffness=[0.5]), (0.0, -0.5, 0.0, 0.2)
    if material == "granular":
        pile, scale = sim.initial_pile(rng, (0.3, 0.6))
        return sim.PileScene.from_piles([pile], [scale / 2]), (0.0, -1.0, 0.0, -0.7)
    if material == "cloth":
        cloth, l0 = sim.initial_cloth(rng, 4, 5)
        scene = sim.ClothScene.from_cloths([cloth], sf=[0.5], l0=[l0])
        x0, z0 = scene.x[0, 0, 0], scene.x[0, 0, 2]
        return scene, (x0, z0, x0 + 0.3, z0)
    size, com, angle = sim.initial_box(rng)
    return sim.BoxScene.from_boxes([size], [com], [angle]), (0.0, -2.0, 0.0, -1.7)


@pytest.mark.parametrize("material", ["rope", "granular", "cloth", "box"])
def test_sim_env_steps_on_the_host(material):
    scene, segment = _scene(material)
    params = sim.dataclasses.replace(sim_env.SIMULATORS[material][0], settle=4)
    env = sim_env.SimEnv(material, scene, configs.task_config(material), device=None, params=params)
    before = np.array(env.scene.x)
    done = env.step(segment, decoded=True)
    assert done.shape == (4,) and done.dtype == np.float32
    assert env.scene.x.shape == before.shape and np.isfinite(env.scene.x).all()
    host = sim_env.SIMULATORS[material][1](scene, np.asarray(segment, np.float32)[None], params)
    if material == "box":
        assert np.array_equal(env.scene.pose, host[-2]) and np.array_equal(env.scene.x, host[0][:, int(host[3][0]) - 1])
    else:
        assert np.array_equal(env.scene.x, host[-2]) and np.array_equal(env.scene.v, host[-1])


def _digest_tool():
    spec = importlib.util.spec_from_file_location("gen_datagen_digests", os.path.join(ROOT, "tools", "gen_datagen_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("material", ["rope", "granular", "cloth", "box"])
def test_datasets_match_the_recorded_digests(material):
    with open(os.path.join(ROOT, "tests", "golden", "datagen_digests.json")) as f:
        want = json.load(f)[material]
    got = _digest_tool().digests([material])[material]
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}
