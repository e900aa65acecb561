"""Digests of four small host-path datasets, one per material (CPU only, a few seconds):

    python tools/gen_datagen_digests.py            writes tests/golden/datagen_digests.json

Every material: 2 episodes x 2 pushes, seed 3, device=None, settle 8 on the material's default parameters.  Per material the sha256 of every text
file's bytes by relative path, and the sha256 of dtype, shape and bytes of every array in positions.pkl, of every property_params.pkl value and of
the box's .npy files -- array contents, not pickle bytes, so the fixture does not depend on numpy's pickling.  tests/test_sim_surface.py holds
`adaptigraph_amd.datagen` to the committed file; regenerate it only for a change that is MEANT to alter the datasets.
"""
import dataclasses
import hashlib
import json
import os
import pickle
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "datagen_digests.json")


def cases():
    """{material: (generate function, its keyword arguments)}"""
    from adaptigraph_amd import datagen, sim
    short = lambda params: dataclasses.replace(params, settle=8)
    return {"rope": (datagen.generate_rope_dataset, dict(params=short(sim.DEFAULT), n_particles=12)),
            "granular": (datagen.generate_granular_dataset, dict(params=short(sim.PILE_DEFAULT), area_range=(0.3, 0.6))),
            "cloth": (datagen.generate_cloth_dataset, dict(params=short(sim.CLOTH_DEFAULT), grid=(4, 6))),
            "box": (datagen.generate_box_dataset, dict(params=short(sim.BOX_DEFAULT), push_length=1.0))}


def value_digest(value):
    a = np.asarray(value)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def tree_digests(root):
    """{relative path (and key inside a pickle): sha256} over every file under `root`."""
    out = {}
    for folder, _, files in os.walk(root):
        for name in files:
            path = os.path.join(folder, name)
            rel = os.path.relpath(path, root).replace(os.sep, "/")
            if name.endswith(".txt"):
                with open(path, "rb") as f:
                    out[rel] = hashlib.sha256(f.read()).hexdigest()
            elif name.endswith(".npy"):
                out[rel] = value_digest(np.load(path))
            elif name == "positions.pkl":
                with open(path, "rb") as f:
                    for key, arrays in pickle.load(f).items():
                        for e, a in enumerate(arrays):
                            out[f"{rel}:{key}[{e}]"] = value_digest(a)
            elif name == "property_params.pkl":
                with open(path, "rb") as f:
                    for key, value in pickle.load(f).items():
                        out[f"{rel}:{key}"] = value_digest(value)
            else:
                raise RuntimeError(f"a file no digest is defined for: {rel}")
    return dict(sorted(out.items()))


def digests(materials=None):
    out = {}
    for material, (generate, kwargs) in cases().items():
        if materials is None or material in materials:
            with tempfile.TemporaryDirectory() as tmp:
                generate(tmp, 2, 2, seed=3, device=None, **kwargs)
                out[material] = tree_digests(tmp)
    return out


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)
