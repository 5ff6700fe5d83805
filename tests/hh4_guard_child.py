"""Child process of tests/test_gpu_hh4.py: the small MODE_HH4 parity cases in all three schedules with the engine's
guarded allocation mode on (SGM_DEBUG_ALLOC=1: every device buffer ends at the end of its mapping).  A parity run: a
read or write past the one-role band record ends THIS process, not the test session.  Prints `HH4_GUARD_OK <cases>`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import test_gpu_hh4 as T

    n = 0
    for case in T.CASES:
        for schedule in (0, 1, 2):
            T.check_stages(case, schedule)
            n += 1
    print(f"HH4_GUARD_OK {n}", flush=True)


if __name__ == "__main__":
    main()
