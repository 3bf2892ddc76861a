"""CPU (-m "not gpu"): the poison runs of poison_checks.py through the host-emulation build of the stage code.  The same runs go through
the HIP library in test_gpu_poison.py."""
import poison_checks as PC


def test_face_ignores_poisoned_metric_entries():
    assert PC.check_face("emul") > 0


def test_cube_ignores_poisoned_metric_entries():
    assert PC.check_cube("emul") > 0
