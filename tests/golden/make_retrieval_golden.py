"""Writes tests/golden/retrieval_small.npz: a ring scene of 12 images (K = 48, D = 32, step 12, noise 0.05, seed 11) through
tests/retr_ref.py with C = 8 centroids, 5 Lloyd steps on every row and k = 3 -- the scene, the centroids after every step, the
assignments of all rows, G, sim, the neighbours and the pairs.  Run from the repository root: python tests/golden/make_retrieval_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import retr_ref  # noqa: E402

N, K, D, STEP, NOISE, SEED, C, STEPS, TOPK, FIRST = 12, 48, 32, 12, 0.05, 11, 8, 5, 3, 100


def make():
    scene = retr_ref.ring_scene(N, K, D, STEP, NOISE, SEED)
    cents = retr_ref.train(scene, None, C, STEPS, 1)
    mu = cents[-1]
    a = np.stack([retr_ref.assign(scene[i], mu) for i in range(N)])
    G = retr_ref.encode(scene, None, mu)
    sim = retr_ref.similarity(G, D)
    nbr = retr_ref.top_k(sim, TOPK)
    return dict(scene=scene, centroids=np.stack(cents), assign=a, G=G, sim=sim, nbr=nbr, pairs=retr_ref.pairs(nbr, FIRST),
                params=np.array([N, K, D, STEP, SEED, C, STEPS, TOPK, FIRST], np.int32), noise=np.float64(NOISE))


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "retrieval_small.npz"), **make())
