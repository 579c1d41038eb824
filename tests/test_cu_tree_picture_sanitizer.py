"""tests/sanitize_cu_tree_picture.cpp, a stand-alone program over the host twin of the coding tree over whole pictures (DESIGN.md
section 5r), under AddressSanitizer + UBSan on the CPU (built and run the way tests/test_cu_tree_sanitizer.py builds and runs its
program; nothing is loaded into Python under a sanitizer)."""
import os
import subprocess


def test_sanitizer_program(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    csrc = os.path.join(root, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_cu_tree_picture")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(root, "include"), os.path.join(here, "sanitize_cu_tree_picture.cpp"),
                        os.path.join(csrc, "pnn_cu_tree.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_cu_tree_picture: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
