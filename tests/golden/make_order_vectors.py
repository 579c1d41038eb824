"""Writes tests/golden/f32_order6_vectors.npz: the exact-f32 order model's (oracle/pnn_order.c) float32 predictions for a few blocks of
each of the eight architectures, with the tag of the order and the seeds and shapes that regenerate the inputs (tests/util.py).
A later change to the order contract shows up as a diff of this file; tests/test_order_model.py checks that the model still
reproduces it bit for bit.

    python tests/golden/make_order_vectors.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pnn_oracle as O   # noqa: E402
from tests import util                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f32_order6_vectors.npz")
ARCHS = [(True, 4), (True, 8), (True, 16), (False, 4), (False, 8), (False, 16), (False, 32), (False, 64)]
N_BLOCKS = {4: 6, 8: 6, 16: 4, 32: 3, 64: 2}


def inputs(is_fc, w, seed, n):
    params = util.make_params(w, is_fc, seed, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, n, seed + 1, masked_fraction=0.5)
    return params, above, left


def forward(is_fc, w, params, above, left):
    if is_fc:
        return O.order_fc_forward(params, w, util.flatten_fc(above, left))
    return O.order_conv_forward(params, w, above, left)


def main():
    O.build()
    d = {"tag": np.array(O.order_tag())}
    for i, (is_fc, w) in enumerate(ARCHS):
        name = "%s%d" % ("fc" if is_fc else "conv", w)
        seed, n = 7100 + 10 * i, N_BLOCKS[w]
        params, above, left = inputs(is_fc, w, seed, n)
        d[name + "_seed"] = np.int64(seed)
        d[name + "_n"] = np.int64(n)
        d[name + "_out"] = forward(is_fc, w, params, above, left)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
