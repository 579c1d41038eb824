"""Generator of tests/golden/hm_transforms.npz: recorded inputs and outputs of HM's own transforms, the free functions xTrMxN and
xITrMxN of TComTrQuant.cpp (8-bit video, maxLog2TrDynamicRange 15, useDST at 4 x 4), for tests/test_trquant.py.

    python tests/golden/make_hm_transforms.py /path/to/hm_16_15_regular [build directory]

compiles tests/golden/hm_transforms_shim.cpp together with the tree's TComTrQuant.cpp and TComRom.cpp BY PATH into the build directory
(a temporary one by default; the class members the two free functions never reach stay unresolved and unreferenced), pipes the blocks
through it and writes the fixture.  Only the fixture is kept: recorded numbers, no code.

Blocks per T in {4, 8, 16, 32}, as (prediction, target) uint8 pairs so that the test can feed them through transform_stages: the extremes
(prediction 0 / target 255, the reverse, the checkerboard), random and smooth pairs of tests/trquant_cases.py.  Forward: residual ->
'coeffs'.  Inverse: the dequantised coefficients the numpy restatement of tests/trquant_cases.py derives from HM's 'coeffs' at the QPs
of 'qps' -> 'residual'; the test checks that the host twin feeds its inverse the same 'dequant' before it compares the outputs.
Arrays of one T: predictions_T, targets_T uint8 [n, T, T]; coeffs_T int16 [n, T, T]; dequant_T, residual_T int16 [nb_qps, n, T, T]."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import trquant_cases as cases  # noqa: E402

QPS = (0, 22, 37)
# HM's documented default, TypeDef.h's "0 (default)": int coefficients and, which is what matters here, the standard's 6-bit matrices in
# BOTH directions.  A tree whose TypeDef.h sets the switch to 1 multiplies by 14-bit "high precision" matrices in the FORWARD transform
# (RExt__HIGH_PRECISION_FORWARD_TRANSFORM; its coefficients differ from the standard-matrix ones by a few units); the inverse transform,
# the normative half, is the same either way.  include/pnn_hip.h defines the forward transform by the standard's matrix.
HM_DEFAULT_TYPES = "-DRExt__HIGH_BIT_DEPTH_SUPPORT=0"
NB_BLOCKS = {4: 48, 8: 48, 16: 36, 32: 24}


def build(hm_tree, build_dir):
    lib = os.path.join(hm_tree, "source", "Lib")
    exe = os.path.join(build_dir, "hm_transforms_shim")
    subprocess.check_call(["g++", "-O1", "-w", "-std=c++11", "-ffunction-sections", "-fdata-sections", "-I" + lib, HM_DEFAULT_TYPES,
                           os.path.join(HERE, "hm_transforms_shim.cpp"), os.path.join(lib, "TLibCommon", "TComTrQuant.cpp"),
                           os.path.join(lib, "TLibCommon", "TComRom.cpp"), "-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all",
                           "-o", exe])
    return exe


def run(exe, direction, blocks):
    """HM's transform of int blocks [n, T, T]"""
    n, t = blocks.shape[0], blocks.shape[1]
    records = b"".join(np.array([direction, t], np.int32).tobytes() + np.ascontiguousarray(b, np.int32).tobytes() for b in blocks)
    out = subprocess.run([exe], input=records, stdout=subprocess.PIPE, check=True).stdout
    return np.frombuffer(out, np.int32).reshape(n, t, t)


def main():
    hm_tree = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(hm_tree, sys.argv[2] if len(sys.argv) > 2 else tmp)
        arrays = {"qps": np.array(QPS, np.int32)}
        for t, n in NB_BLOCKS.items():
            predictions, targets = cases.mixed_pairs(t, n, 900 + t)
            coeffs = run(exe, 0, targets.astype(np.int32) - predictions.astype(np.int32))
            dequant = np.stack([np.stack([cases.dequantise(cases.quantise(c.astype(np.int64), qp)[0], qp, t.bit_length() - 1) for c in coeffs])
                                for qp in QPS])
            residual = np.stack([run(exe, 1, d) for d in dequant])
            for a in (coeffs, dequant, residual):
                assert np.abs(a).max() <= 32768 and a.min() >= -32768 and a.max() <= 32767
            arrays.update({"predictions_%d" % t: predictions, "targets_%d" % t: targets, "coeffs_%d" % t: coeffs.astype(np.int16),
                           "dequant_%d" % t: dequant.astype(np.int16), "residual_%d" % t: residual.astype(np.int16)})
    path = os.path.join(HERE, "hm_transforms.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
