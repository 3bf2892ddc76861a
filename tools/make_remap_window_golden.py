"""Writes tests/golden/remap_window/*.npz: the results of the vertical remap on the states of tests/test_emul_remap_window.py, from the
host-emulation library given on the command line (g++ -O2 -std=c++17 -fPIC -DFV3LM_HOST_EMUL -shared csrc/fv3lm_capi.cpp).  The committed
goldens come from the library of the commit before the remap read its source levels through a window; test_emul_remap_window.py demands
np.array_equal with them from the current build.

    python tools/make_remap_window_golden.py path/to/libfv3lm_emul.so"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    lib = os.path.abspath(sys.argv[1])
    import common
    common.build_emul = lambda: lib      # the library under tests/_emul is rebuilt from the current sources; this one is taken as it is
    import test_emul_remap_window as W
    os.makedirs(W.GOLDEN, exist_ok=True)
    for name in W.CASES:
        c = W.make_case(name)
        S = W.make_state(c, name)
        out = {}
        for last in (0, 1):
            out.update(W.bits(c, S, last))
        path = os.path.join(W.GOLDEN, name + ".npz")
        np.savez(path, **out)
        print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
