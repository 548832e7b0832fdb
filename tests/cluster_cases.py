"""Inputs of the clustering tests: graphs whose shape is chosen directly, and a small protein set with families in it."""
import numpy as np


def family_set(seed=2718, ancestors=5, n=60, loners=8):
    """About n protein code arrays of 30 .. 200 residues: mutated copies and fragments of a handful of random ancestors, and a few
    unrelated sequences.  Returns (codes, family) with family[i] the ancestor's number, or -1 for an unrelated sequence."""
    rng = np.random.default_rng(seed)
    roots = [rng.integers(0, 20, size=int(rng.integers(120, 201))).astype(np.uint8) for _ in range(ancestors)]
    codes, family = [], []
    for i in range(n - loners):
        a = int(rng.integers(0, ancestors))
        s = roots[a].copy()
        if rng.random() < 0.5:                                       # a fragment
            width = int(rng.integers(30, len(s)))
            first = int(rng.integers(0, len(s) - width + 1))
            s = s[first:first + width]
        rate = float(rng.choice([0.05, 0.2, 0.4, 0.6]))
        hit = rng.random(len(s)) < rate
        s[hit] = rng.integers(0, 20, size=int(hit.sum())).astype(np.uint8)
        codes.append(s)
        family.append(a)
    for i in range(loners):
        codes.append(rng.integers(0, 20, size=int(rng.integers(30, 201))).astype(np.uint8))
        family.append(-1)
    order = rng.permutation(len(codes))
    return [codes[i] for i in order], [family[i] for i in order]


def scrambled_path(n, seed=99):
    """a path over n nodes whose numbering is a fixed permutation: edges (perm[i], perm[i + 1])"""
    perm = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    return perm[:-1].copy(), perm[1:].copy()
