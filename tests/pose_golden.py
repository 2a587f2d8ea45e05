"""Reader of tests/golden/bone_mask.npz (written by tests/golden/make_golden_bone_mask.py from the reference's own
create_mask and HumanPoseDataset), shared by the CPU and GPU pose tests."""
import os
import pickle

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bone_mask.npz")
EDGE_FRAME = 3               # the last frame of each 64-pixel case: behind-camera joint, keypoints across the borders


def load():
    return np.load(PATH)


def bits(g, key, shape=None):
    shape = tuple(g[key.replace("_bits", "_shape")]) if shape is None else shape
    return np.unpackbits(g[key])[:int(np.prod(shape))].reshape(shape).astype(np.float32)


def cases(g):
    """(name, poses, K, size, thickness, golden {mask, keypoint_mask, disparity, joint_pos})"""
    for c in g["cases"]:
        c = str(c)
        dtype, size, t = c.split("_")
        yield (c, g[f"{c}_poses"], g[f"{c}_K"], int(size), float(t[1:]),
               {"mask": bits(g, f"{c}_mask_bits"), "keypoint_mask": bits(g, f"{c}_keypoint_mask_bits"),
                "disparity": g[f"{c}_disparity"], "joint_pos": g[f"{c}_joint_pos"]})


def write_cache(g, name, directory):
    """the golden's pose-only cache.pickle (and canonical.npy) into `directory`"""
    prefix = f"{name}__"
    d = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    with open(os.path.join(directory, "cache.pickle"), "wb") as f:
        pickle.dump(d, f)
    if f"{name}_canonical" in g.files:
        np.save(os.path.join(directory, "canonical.npy"), g[f"{name}_canonical"])
    return d


def items(g, name):
    """{index: {key: golden value}} of the reference's HumanPoseDataset items"""
    out = {}
    for i in g["dataset_items"]:
        i = int(i)
        pre = f"{name}_item{i}_"
        it = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
        it["bone_mask"] = bits(g, pre + "bone_mask_bits", (64, 64))
        del it["bone_mask_bits"]
        out[i] = it
    return out
