"""TEST INFRASTRUCTURE ONLY -- the dirty-workspace runs of
tests/carryover_util.py as a program, so that tests/test_gpu_carryover.py can
repeat them under the library's launch-time knobs (read once per process):

  CFWS_PLAN_SINGLE=0      the 524,289-frame plans as reduce / scan / apply
  CFWS_FUSED_DESER=0      the fused receive's shapes as plan + execute
  CFWS_SMALL=0            the small batches on the general path
  CFWS_H2_UNITS_MERGED=0  the HTTP/2 receive's layout and units as two launches
  CFWS_SER_INREG=0        the send's edge chunks always by the edge workgroups

Arguments: case-name prefixes (none: every case). Each named case runs over
a workspace of 0x00, 0xFF, 0xAA, 0x55 and of what the same entry point left
there after another batch; every output is compared with the oracle and with
the first run. Prints "CARRYOVER OK".
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import carryover_util as U  # noqa: E402
from coldforce_amd import cfws  # noqa: E402


def main():
    cfws.init()
    prefixes = sys.argv[1:]
    names = [n for n in U.CASE_NAMES if not prefixes or any(n.startswith(p) for p in prefixes)]
    assert names, f"no case matches {prefixes}"
    for name in names:
        case = U.cases()[name]
        U.run_dirty(case)
        case.release()
        print("ok", name, flush=True)
    print("CARRYOVER OK", len(names), {k: v for k, v in os.environ.items() if k.startswith("CFWS_")}, flush=True)


if __name__ == "__main__":
    main()
