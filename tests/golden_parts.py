"""Golden vectors stored in several files: tests/golden/<stem>.npz plus <stem>.part0.npz,
<stem>.part1.npz, ... (tools/gen_golden.py splits a set that would exceed 1 MiB in one file).
An array whose name appears in more than one file was cut along axis 0 and is joined again in
file order; every other array is taken as it is."""
import glob
import os
import re

import numpy as np


def load_golden(path: str) -> dict:
    stem = path[:-len(".npz")]
    parts = sorted(glob.glob(glob.escape(stem) + ".part*.npz"),
                   key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    chunks = {}
    for p in [path] + parts:
        with np.load(p, allow_pickle=False) as d:
            for k in d.files:
                chunks.setdefault(k, []).append(d[k])
    return {k: v[0] if len(v) == 1 else np.concatenate(v, 0) for k, v in chunks.items()}
