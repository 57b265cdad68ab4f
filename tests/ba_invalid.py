"""Scenes, sizes and options shared by tests/test_ba_invalid_ref.py (CPU: the oracle does what the cases are here for) and
tests/test_ba_invalid_gpu.py (GPU against the oracle): LM steps that are invalid for ONE reason each -- a singular landmark block
(synth_ba.make_lone_landmark_scene) or a reduced camera system that breaks down in the factorisation (synth_ba.make_dead_camera_scene,
the dead camera first or last among the free ones) -- at reduced dimensions that finish the reduced system in different ways.

All with intrinsics_mode = 0 and fix_cam0_pose = 1: camera 0 has no column, every other camera six (camera 1 three where its
translation is fixed)."""
import functools

from oracle import orc_ba
from reconstructor_amd import synth_ba

# reduced dimension -> (cameras, fix_cam1_translation): 384 = 3 x 128, no padding and the unfused finish; 132, padded to 256, and 27, one
# block, the fused finish
SIZES = {384: (65, 0), 132: (23, 0), 27: (6, 1)}
KINDS = ("lone", "dead_first", "dead_last")
INTEGERS = ("termination", "iterations", "invalid_steps", "successful_steps", "unsuccessful_steps", "reduced_dim")


@functools.lru_cache(maxsize=None)
def scene(kind, n):
    nc = SIZES[n][0]
    if kind == "lone":
        return synth_ba.make_lone_landmark_scene(nc)
    return synth_ba.make_dead_camera_scene(nc, 1 if kind == "dead_first" else nc - 1)


def set_options(o, n, floor=None, limit=None):
    """the structure of the cases on top of the defaults `o`; floor: min_lm_diagonal (None: the default, 1e-6), limit:
    max_consecutive_invalid_steps (None: the default, 5)"""
    o.intrinsics_mode, o.fix_cam0_pose, o.fix_cam1_translation = 0, 1, SIZES[n][1]
    if floor is not None:
        o.min_lm_diagonal = floor
    if limit is not None:
        o.max_consecutive_invalid_steps = limit
    return o


@functools.lru_cache(maxsize=None)
def oracle(kind, n, floor=None, limit=None):
    """(poses, intrinsics, points, summary) of the CPU oracle, solved once per case and shared: read only"""
    o = set_options(orc_ba.default_options(SIZES[n][0]), n, floor, limit)
    return orc_ba.solve(scene(kind, n), options=o, threads=4)
