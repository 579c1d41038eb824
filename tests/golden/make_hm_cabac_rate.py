"""Generator of tests/golden/hm_cabac_rate.npz: numbers recorded from HM-16.15's own residual entropy coding, for
tests/test_cabac_rate.py.

    python tests/golden/make_hm_cabac_rate.py /path/to/hm_16_15_regular [build directory]

compiles tests/golden/hm_cabac_rate_shim.cpp together with the tree's ContextModel.cpp, TComTrQuant.cpp and TComRom.cpp BY PATH into the
build directory (a temporary one by default; what the called functions never reach stays unresolved and unreferenced), runs it and writes
the fixture.  Only the fixture is kept: recorded numbers, no code.

WHAT IS PINNED.  The pieces of codeCoeffNxN that HM exposes without a coding unit: ContextModel::init -> getEntropyBits / update along
200-bin sequences that reach all 126 states (per QP 0, 22, 37, 51 and each of the 80 luma contexts, from its I-slice init value, which is recorded too), the scan
tables of initROM, getSigCtxInc over every position, pattern and scan, getSigCoeffGroupCtxInc and calcPatternSigCtx over 4 x 4 group
maps, g_uiGroupIdx and getLastSignificantContextParameters.  WHAT IS NOT, HERE: the bits of a whole TEncSbac::codeCoeffNxN call on a
TEncBinCABACCounter -- that needs a TComSPS / TComPPS / TComSlice and a one-CU TComDataCU / TComTU stood up around it.  That is what
tests/golden/make_hm_unit_coding.py does: the ORDER in which codeCoeffNxN strings these pieces together (which flags are coded or
inferred, the c1 walk, the Rice parameter, the escape codes, the hidden sign) is pinned by its fixture, to which the restatement of
tests/cabac_rate_cases.py is held as well.  Still pinned nowhere: cbf_luma, mode bits, the running contexts of a slice, RDOQ."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HM_DEFAULT_TYPES = "-DRExt__HIGH_BIT_DEPTH_SUPPORT=0"
NB_CTX = 80


def build(hm_tree, build_dir):
    lib = os.path.join(hm_tree, "source", "Lib")
    exe = os.path.join(build_dir, "hm_cabac_rate_shim")
    subprocess.check_call(["g++", "-O1", "-w", "-std=c++11", "-ffunction-sections", "-fdata-sections", "-I" + lib, HM_DEFAULT_TYPES,
                           os.path.join(HERE, "hm_cabac_rate_shim.cpp")] +
                          [os.path.join(lib, "TLibCommon", name) for name in ("ContextModel.cpp", "TComTrQuant.cpp", "TComRom.cpp")] +
                          ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def main():
    hm_tree = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(hm_tree, sys.argv[2] if len(sys.argv) > 2 else tmp)
        text = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode()
    raw = {}
    for line in text.splitlines():
        name, count, *values = line.split()
        assert int(count) == len(values)
        raw[name] = np.array(values, np.int64)
    arrays = {"qps": np.array((0, 22, 37, 51), np.int32), "init_values": raw.pop("init_values").astype(np.uint8)}
    assert arrays["init_values"].size == NB_CTX
    arrays["model_bins"] = raw.pop("model_bins").astype(np.uint8).reshape(NB_CTX, -1)
    k = arrays["model_bins"].shape[1]
    arrays["model_bits"] = raw.pop("model_bits").astype(np.int32).reshape(4, NB_CTX, k)
    arrays["model_states"] = raw.pop("model_states").astype(np.uint8).reshape(4, NB_CTX, k)
    arrays["group_maps"] = raw.pop("group_maps").astype(np.uint8).reshape(-1, 4, 4)
    arrays["group_ctx"] = raw.pop("group_ctx").astype(np.uint8).reshape(-1, 4, 4)
    arrays["group_pattern"] = raw.pop("group_pattern").astype(np.uint8).reshape(-1, 4, 4)
    arrays["last_group"] = raw.pop("last_group").astype(np.uint8)
    arrays["last_params"] = raw.pop("last_params").astype(np.uint8).reshape(4, 2)
    for name, values in raw.items():
        arrays[name] = values.astype(np.uint16).reshape(4, -1) if name.startswith("sig_ctx") else values.astype(np.uint16)
    path = os.path.join(HERE, "hm_cabac_rate.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
