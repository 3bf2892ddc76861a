"""CPU (-m "not gpu"): the fused a2b_ord4 launch of the host-emulation build against the staged launches (fused_checks.py):
step_tl bit for bit, step_ad to 1e-13.  The same cases run on the MI355X in test_gpu_a2b_fused.py."""
from common import Case, CubeCase
from fused_checks import check_fused_equals_staged


def test_fused_a2b_periodic_tile_many_blocks():
    # 71 x 21 corner points: 2 x 2 blocks, a thin last block column and a second block row
    check_fused_equals_staged("emul/periodic", lambda: Case(nx=70, ny=20, npz=3, n_split=2, k_split=1, dt=900.0, backend="emul", oracle=False, nq=1), "FV3LM_A2B_FUSED")


def test_fused_a2b_cube_faces_rim_strips_corners():
    # six C66 faces: a 63 x 63 bulk of 1 x 4 blocks beside the rim, the strips and the corners
    check_fused_equals_staged("emul/cube", lambda: CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="emul", nq=1), "FV3LM_A2B_FUSED")


def test_fused_a2b_nonhydrostatic_interfaces():
    # non-hydrostatic: nh_p_grad runs a2b_ord4 on npz and on npz+1 levels
    check_fused_equals_staged("emul/nh", lambda: Case(nx=66, ny=18, npz=3, n_split=1, k_split=1, dt=300.0, backend="emul", oracle=False, hydrostatic=0), "FV3LM_A2B_FUSED")


def test_fused_a2b_subface_windows():
    # six C136 faces cut 2 x 2: 68-wide windows, each with one cube corner, two cube edges and two interior boundaries
    check_fused_equals_staged("emul/windows", lambda: CubeCase(n=136, npz=2, n_split=1, k_split=1, dt=100.0, backend="emul", nq=1, layout=2), "FV3LM_A2B_FUSED")
