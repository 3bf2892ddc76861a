"""CPU: tests/remap_window_host.cpp, compiled here with g++ -O2 -std=c++17 -DFV3LM_HOST_EMUL and run.  It drives map_col, map_col_lim and
map_col_ad_s of csrc/remap.h and the plain form they were derived from (every probe loads from the functors again) through functors over
small arrays, km = 12 and 127, and demands memcmp equality of the outputs, of every workspace vector that survives the call and of the
three adjoint output streams, on +-3 % layers, the 'large' warp, tied interfaces and two unordered columns (target top above the source
top: the not-found path; target bottom below the last source interface: no bottom layer), which fv3lm_remap cannot reach.  On the ordered
columns it counts the functor calls: forward pe1 <= 2 (km + 1) + 8 and q1 <= km + 8, adjoint pe1 <= 3 (km + 1) + 8 and q1 <= 3 km + 8
(the plain form: 9.0 km / 3.0 km and 11.0 km / 4.0 km)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "fv3_jedi_linearmodel_amd", "csrc")


def test_window_is_bit_identical_to_the_plain_form(tmp_path):
    exe = str(tmp_path / "remap_window_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFV3LM_HOST_EMUL", "-I", CSRC, os.path.join(HERE, "remap_window_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all columns bit-identical" in r.stdout
