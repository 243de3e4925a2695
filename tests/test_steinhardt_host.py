"""The exact Steinhardt yardstick (tests/_steinhardt_ref.py) against the CPU oracle and against the textbook values — no GPU.

This is also where the bounds of tests/test_gpu_steinhardt.py are measured: every test prints the oracle's largest absolute
error per kind of output, and asserts that it is within ``_steinhardt_ref.ORACLE_ERR`` — the figures the GPU bounds are 64
times of.  (pytest -s shows the figures; docs/NOTEBOOK.md records them.)"""
import numpy as np
import pytest

import _steinhardt_cases as SC
import _steinhardt_ref as R
from mdapy_amd.build_lattice import lattice_positions
from oracle import oracle as O


def _within(err, what):
    print(f"steinhardt oracle-vs-exact {what}: " + ", ".join(f"{k} {e:.2e}" for k, e in err.items()))
    for k, e in err.items():
        assert e <= R.ORACLE_ERR[k], f"{what}: the oracle's {k} is {e:.3g} from exact, recorded worst {R.ORACLE_ERR[k]:.3g}"


@pytest.mark.parametrize("entry", SC.LISTS, ids=[SC.list_id(e) for e in SC.LISTS])
@pytest.mark.parametrize("name", SC.CASES)
def test_oracle_against_exact(name, entry):
    _within(SC.measure(O, SC.case(name), entry), f"{name} {entry[0]}")


def test_oracle_against_exact_high_degree():
    _within(SC.measure(O, SC.case("fcc256"), SC.HIGH_DEGREE), "fcc256 [16]")


def test_bounds_follow_from_the_recorded_errors():
    assert R.BOUND == {k: 64 * e for k, e in R.ORACLE_ERR.items()}
    assert all(0.0 < b <= R.CEILING == 1e-12 for b in R.BOUND.values())


# q4, q6, w4-hat, w6-hat of the perfect lattices (Steinhardt, Nelson, Ronchetti, PRB 28, 784 (1983); Mickel et al.,
# J. Chem. Phys. 138, 044501 (2013), table I), q_l in closed form where it has a short one
TEXTBOOK = {
    "fcc": (12, np.sqrt(7 / 192), np.sqrt(169 / 512), -0.159317, -0.013161),
    "bcc": (8, np.sqrt(7 / 27), np.sqrt(32 / 81), -0.159317, 0.013161),
    "hcp": (12, 7 / 72, 0.484762, 0.134097, -0.012442),
    "sc": (6, np.sqrt(7 / 12), np.sqrt(1 / 8), 0.159317, 0.013161),
}


@pytest.mark.parametrize("structure", list(TEXTBOOK))
def test_perfect_lattices_give_the_textbook_values(structure):
    k, q4, q6, w4, w6 = TEXTBOOK[structure]
    pos, box = lattice_positions(structure, 3.0, 4, 4, 4)
    org = np.zeros(3)
    x, y, z = SC._xyz(pos)
    v = np.zeros((len(x), k), np.int32); d = np.zeros((len(x), k))
    O.knn(x, y, z, box, org, SC.PBC, k, v, d, 2)
    n = np.full(len(x), k, np.int32)
    exact = R.exact_columns(R.Bonds(x, y, z, box, org, SC.PBC, v, d, n, k, 1e9), [4, 6])
    qr = np.zeros((len(x), 2, 13)); qi = np.zeros_like(qr); qn = np.zeros((len(x), 6))
    O.get_sq(x, y, z, box, org, SC.PBC, v, d, n, np.zeros((2, 2)), np.array([4, 6], np.int32), k, 6, True, True, False, False, 1e9, False, qr, qi, qn, 1)
    want = np.array([q4, q6, w4, w6])
    for who, have in (("exact", np.stack([exact["ql"][:, 0], exact["ql"][:, 1], exact["wlh"][:, 0], exact["wlh"][:, 1]], axis=1)),
                      ("oracle", qn[:, [0, 1, 4, 5]])):
        off = np.abs(have - want).max(axis=0)
        print(f"steinhardt textbook {structure} {who}: q4 {have[0, 0]:.6f} q6 {have[0, 1]:.6f} w4^ {have[0, 2]:.6f} w6^ {have[0, 3]:.6f}")
        # closed forms to rounding, values published to six decimals to half a unit of the last one
        assert (off <= np.array([1e-12, 5e-7 if structure == "hcp" else 1e-12, 5e-7, 5e-7])).all(), (who, off)


@pytest.mark.parametrize("slot", SC.SLOTS, ids=[f"q6index{s[0]}" for s in SC.SLOTS])
def test_oracle_solid_liquid_equals_the_exact_rule(slot):
    for name, c in SC.solid_liquid_cases():
        SC.check_solid_liquid(O, name, c, slot)


def test_get_sq_refuses_bad_arguments():
    """mdh_get_sq checks its arguments before it touches the device: each of these raises, on a machine without a GPU too"""
    from mdapy_amd import _sbo

    c = SC.case("n65")

    def run(llist, lmax, use_weight=False, weight=np.zeros((2, 2))):
        qr = np.zeros((c.N, len(llist), 2 * lmax + 1)); qi = np.zeros_like(qr); qn = np.zeros((c.N, len(llist)))
        _sbo.get_sq(c.x, c.y, c.z, c.box, c.org, c.bnd, c.v, c.d, c.n, weight, np.array(llist, np.int32), 0, lmax, False, False, False, False,
                    c.rc, use_weight, qr, qi, qn, 1)

    for bad, message in ((dict(llist=[4, 6], lmax=4), "0 <= l <= lmax"), (dict(llist=[-1], lmax=2), "0 <= l <= lmax"),
                         (dict(llist=[2] * 17, lmax=2), "len.llist. <= 16"), (dict(llist=[41], lmax=41), "lmax <= 40"),
                         (dict(llist=[4], lmax=4, use_weight=True, weight=None), "without weight array")):
        with pytest.raises(ValueError, match=message):
            run(**bad)
