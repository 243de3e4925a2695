"""The Steinhardt kernels of mdapy_amd/csrc/sbo.hip against exact mathematics (tests/_steinhardt_ref.py: scipy's spherical
harmonics, sympy's 3j symbols), through ``_sbo.get_sq`` and ``_sbo.identifySolidLiquid`` on lists built by the CPU oracle.

One test id is one system and one degree list; the id names the kernels ``mdh_get_sq`` launches for it, first with w_l,
w_l-hat and averaging all on, then with all off (tests/_steinhardt_cases.py derives them from the launch arithmetic).  Each runs
with and without weights.  q_lm, q_l, w_l and w_l-hat must be within ``_steinhardt_ref.BOUND`` of exact: 64 times the CPU
oracle's own worst error, measured by tests/test_steinhardt_host.py, and never more than 1e-12."""
import contextlib

import numpy as np
import pytest

import _steinhardt_cases as SC
import _steinhardt_ref as R
import mdapy_amd as mp
from mdapy_amd import _lib, _sbo
from mdapy_amd.devarray import as_numpy
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _variant(v):
    _lib.lib().mdh_debug_set_sq_variant(v)
    try:
        yield
    finally:
        _lib.lib().mdh_debug_set_sq_variant(0)


def _within(err, what):
    print(f"steinhardt HIP-vs-exact {what}: " + ", ".join(f"{k} {e:.2e} (bound {R.BOUND[k]:.1e})" for k, e in err.items()))
    for k, e in err.items():
        assert e <= R.BOUND[k], f"{what}: {k} is {e:.3g} from exact, bound {R.BOUND[k]:.3g}"


@pytest.mark.parametrize("entry", SC.LISTS, ids=[SC.list_id(e) for e in SC.LISTS])
@pytest.mark.parametrize("name", SC.CASES)
def test_get_sq_against_exact(name, entry):
    with _variant(entry[2]):
        err = SC.measure(_sbo, SC.case(name), entry)
    _within(err, f"{name} {entry[0]}")


def test_get_sq_against_exact_high_degree():
    _within(SC.measure(_sbo, SC.case("fcc256"), SC.HIGH_DEGREE), "fcc256 [16]")


@pytest.mark.parametrize("entry", SC.LISTS[:1] + SC.LISTS[12:13], ids=["pair", "generic"])
def test_atom_without_neighbours_has_the_oracles_nan_and_inf_pattern(entry):
    """one atom, no neighbour: 0 * (1 / 0) in every q_lm — NaN and inf where the oracle has them, row for row"""
    c = SC.case("single")
    llist, lmax, _ = entry
    for full, use_w in SC.COMBOS:
        want, got = SC.call(O, c, llist, lmax, full, use_w), SC.call(_sbo, c, llist, lmax, full, use_w)
        for a, b in zip(want, got):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
            assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("entry", [SC.LISTS[0], SC.LISTS[1], SC.LISTS[11], SC.LISTS[17], SC.LISTS[19]],
                         ids=[SC.list_id(SC.LISTS[k]) for k in (0, 1, 11, 17, 19)])
@pytest.mark.parametrize("name", ["fcc250_open_z", "tri256"])
def test_get_sq_adds_onto_the_callers_content(name, entry):
    """q_lm arrays that go in holding small random values: the sums start from them and are scaled by 1 / wsum with them, slots
    past a degree's 2l+1 keep them.  HIP against the oracle through the pair, per-degree and generic kernels."""
    c = SC.case(name)
    llist, lmax, variant = entry
    start = np.random.default_rng(9).normal(0.0, 1e-2, (2, c.N, len(llist), 2 * lmax + 1))
    for full, use_w in SC.COMBOS:
        want = SC.call(O, c, llist, lmax, full, use_w, start)
        with _variant(variant):
            got = SC.call(_sbo, c, llist, lmax, full, use_w, start)
        nl = len(llist)
        assert np.abs(want[0] - SC.call(O, c, llist, lmax, full, use_w)[0]).max() > 1e-4  # (the content took part)
        for kind, a, b in (("qlm", want[0], got[0]), ("qlm", want[1], got[1]), ("ql", want[2][:, :nl], got[2][:, :nl])) + \
                ((("wl", want[2][:, nl:2 * nl], got[2][:, nl:2 * nl]), ("wlh", want[2][:, 2 * nl:], got[2][:, 2 * nl:])) if full else ()):
            assert np.array_equal(np.isnan(a), np.isnan(b))
            off = float(np.nanmax(np.abs(a - b), initial=0.0))
            print(f"steinhardt HIP-vs-oracle on content {name} {llist} full={full} weights={use_w} {kind}: {off:.2e}")
            assert off <= R.BOUND[kind], (kind, off)
        for il, l in enumerate(llist):  # untouched slots, bit for bit
            assert np.array_equal(got[0][:, il, 2 * l + 1:], start[0][:, il, 2 * l + 1:]) and np.array_equal(got[1][:, il, 2 * l + 1:], start[1][:, il, 2 * l + 1:])


@pytest.mark.parametrize("slot", SC.SLOTS, ids=[f"q6index{s[0]}" for s in SC.SLOTS])
def test_solid_liquid_equals_the_exact_rule(slot):
    for name, c in SC.solid_liquid_cases():
        SC.check_solid_liquid(_sbo, name, c, slot)


def test_system_columns_against_exact():
    """column names and slot order of System.cal_steinhardt_bond_orientation depend on llist: every column, solidliquid and nbond
    against the exact values on the system's own list"""
    c = SC.case("fcc256")
    llist = [2, 4, 6, 8, 10, 12]
    s = mp.System(pos=np.stack([c.x, c.y, c.z], axis=1), box=c.box)
    s.cal_steinhardt_bond_orientation(llist, rc=SC.RC, wl=True, wlhat=True, average=True, identify_liquid=True)
    cell, frame = s._get_compute_view()
    v, d, n = as_numpy(s.verlet_list), as_numpy(s.distance_list), as_numpy(s.neighbor_number)
    bonds = R.Bonds(*(frame[k].to_numpy() for k in "xyz"), cell.box, cell.origin, cell.boundary, v, d, n, 0, SC.RC)
    exact = R.exact_columns(bonds, llist, None, True)
    for il, l in enumerate(llist):
        for column, kind in ((f"ql{l}", "ql"), (f"wl{l}", "wl"), (f"wlh{l}", "wlh")):
            off = float(np.abs(s.data[column].to_numpy() - exact[kind][:, il]).max())
            print(f"steinhardt System {column}: {off:.2e}")
            assert off <= R.BOUND[kind], (column, off)
    want_sl, want_nb, gap = bonds.solid_liquid(exact["qlm"][:, 2, :13], 0.7, 7)
    assert gap >= 1e-9
    assert np.array_equal(s.data["nbond"].to_numpy(), want_nb) and np.array_equal(s.data["solidliquid"].to_numpy(), want_sl)


def test_entries_of_another_periodic_image_keep_the_references_sine():
    """32 atoms in a box thinner than two bond lengths, 24 nearest: many entries belong to another periodic image than the minimum
    image get_sq forms, so the listed distance is not the length of that vector.  There sin(theta) stays the reference's
    sqrt(1 - cos^2) (rxy / r is for bonds whose length the list holds): HIP against the oracle, pair, per-degree and generic"""
    from mdapy_amd.build_lattice import lattice_positions

    pos, box = lattice_positions("fcc", SC.A_FCC, 2, 2, 2)
    pos = pos + np.random.default_rng(12).normal(0.0, 0.1, pos.shape)
    c = SC._nearest(pos, box, np.zeros(3), SC.PBC, 24, 1e9)
    c.N, c.weight = len(c.x), None
    dr = np.stack([c.x, c.y, c.z], axis=1)[c.v] - np.stack([c.x, c.y, c.z], axis=1)[:, None, :]
    dr -= np.diag(box) * np.floor(dr / np.diag(box) + 0.5)
    foreign = np.abs(np.sqrt((dr * dr).sum(axis=2)) - c.d) > 1e-6
    assert 0.1 < foreign.mean() < 0.9
    for llist, lmax in (([4, 6], 6), ([6], 6), ([4, 9], 9)):
        nl = len(llist)
        want, got = SC.call(O, c, llist, lmax, True, False), SC.call(_sbo, c, llist, lmax, True, False)
        assert np.isfinite(want[2]).all()
        for kind, a, b in (("qlm", want[0], got[0]), ("qlm", want[1], got[1]), ("ql", want[2][:, :nl], got[2][:, :nl]),
                           ("wl", want[2][:, nl:2 * nl], got[2][:, nl:2 * nl]), ("wlh", want[2][:, 2 * nl:], got[2][:, 2 * nl:])):
            off = float(np.abs(a - b).max())
            print(f"steinhardt HIP-vs-oracle foreign images {llist} {kind}: {off:.2e}")
            assert off <= R.BOUND[kind], (kind, off)
