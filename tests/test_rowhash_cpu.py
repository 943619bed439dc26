"""gc_aes.h's row_hash (the fixed part of a label's hash cached across the rows of a multiplier array) and the
lane-uniform hash (one label in the 32 lanes of a half wave), on the host against hash_n: tests/tools/rowhash_host.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_hash_and_lane_uniform_hash_equal_hash_n(tmp_path):
    exe = str(tmp_path / "rowhash_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linreg-mpc_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "tools", "rowhash_host.cpp")])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "rowhash_starts.txt")], stdout=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().splitlines()[-1].startswith("ok:")
