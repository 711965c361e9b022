"""E_SLOPE and E_SPL_STD of tests/test_pull_gradient.py: the errors of the resident splines' first derivative and of the quotient
m'' / m' at the STANDARDISED samples, against the oracle's derivative basis (the method of tools/score_spline_error.py, which
measures the quotient at the raw samples), with the row counts of the finite-difference yardsticks.

Runs on the CPU, on the host test double (which supplies the U section; the numbers are evaluated in NumPy, tests/pull_truth.py -
not by the routine under test).

    python tools/pull_spline_error.py [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(names):
    from tests import pull_truth as pt
    from tests.hostemu import emu
    with emu.install():
        for name in names or pt.CASES:
            tm, om, X, E = pt.build(name)
            _, keep_j, e_fd = pt.jacobian_truth(name, om, X, E)
            _, keep_l, e_l = pt.logdet_truth(name, om, X, E)
            e_slope, e_spl, rows = pt.spline_errors(tm, om, X, E)
            print("    '%s': (%.1e, %.1e),   # (Jacobian: kept %d / %d, e_FD %.1e; quotient: kept %d / %d, own estimate %.1e)"
                  % (name, e_slope, e_spl, int(keep_j.sum()), pt.ROWS, e_fd, int(keep_l.sum()), pt.ROWS, e_l), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
