"""The recipe the fixture generators of tests/golden/ share for asking HM-16.15 itself: ONE shim of this project's own text compiled
together with the tree's sources BY PATH (TLibCommon, the encoder sources make_hm_unit_coding lists, libmd5), sections the shim does
not reach dropped at link time.  tests/golden/make_hm_cu_tree.py and make_hm_cu_tree_picture.py state the same recipe for their
shims; new generators call this one."""
import concurrent.futures
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_hm_transform_skip  # noqa: E402


def build(hm_tree, build_dir, shim):
    """Compiles tests/golden/<shim>.cpp beside the sources of `hm_tree` into build_dir/<shim>; returns the program's path."""
    unit_coding = make_hm_transform_skip.unit_coding
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, shim + ".cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in unit_coding.ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, unit_coding.HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, shim)
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe
