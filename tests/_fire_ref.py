"""A numpy restatement of the FIRE minimizer for its tests, written from the algorithm (FIRE2: Guenole et al. 2020; ABC-FIRE:
Echeverri Restrepo and Andric 2023; the cell as three extra rows: ASE's UnitCellFilter), with the reference's quirks
(src/mdapy/minimizer.py:182-375): the strict ``vf > 0``, the per-component ABC cap behind ``np.all(v)``, the Voigt mask, ``results``
cleared only when a run ends unconverged.

Three layers:

* the fixed-order reductions of include/mdapy_amd.h "_fire" (``tree_sum``, ``tree_dot``) — numpy slices, no fused operations;
* the module-level functions of ``mdapy_amd._fire`` (``dots kick mix move rowmat scatter_rows total``) on numpy arrays, so that the
  module can stand in for ``kernels.fire``;
* ``run(system, ...)``: the whole algorithm on a System's public interface, with the dot product, the row-times-matrix product
  and the treatment of the unstrained positions as parameters."""
import numpy as np

f64 = np.float64
VF, FF, FMAX2, VV, DRDR, ZEROS, ENERGY, VIRIAL, RECORD = 0, 1, 2, 3, 4, 5, 6, 8, 24
MOVE_NORM, MOVE_CAP, MOVE_PLAIN = 0, 1, 2
BLOCK = 256


def _np(a):
    if a is None or isinstance(a, np.ndarray):
        return a
    if hasattr(a, "numpy"):
        return a.numpy()
    return np.asarray(a.to_numpy() if hasattr(a, "to_numpy") else a)


# ------------------------------------------------------------------------------------------------ the fixed-order sums
def _halve(a, combine=np.add):
    """every row of (m, 256): for h = 128 .. 1, entry k < h takes entry k + h; -> entry 0 of every row"""
    a = np.array(a, f64)
    h = BLOCK // 2
    while h >= 1:
        a[:, :h] = combine(a[:, :h], a[:, h:2 * h])
        h //= 2
    return a[:, 0].copy()


def _padded(t):
    t = np.asarray(t, f64).ravel()
    blocks = max(1, -(-len(t) // BLOCK))
    a = np.zeros(blocks * BLOCK)
    a[:len(t)] = t
    return a.reshape(blocks, BLOCK)


def _larger(a, b):
    """the larger of two, a NaN wins"""
    return np.where((a > b) | np.isnan(a), a, b)


def tree_sum(t, combine=np.add):
    """level 1: blocks of 256 consecutive terms, halved.  level 2: partial k starts from 0.0 and takes the block sums k, k + 256, ..
    in turn; the 256 partials are halved"""
    rows = _padded(_halve(_padded(t), combine))
    acc = np.zeros(BLOCK)
    for r in range(rows.shape[0]):
        acc = combine(acc, rows[r])
    return float(_halve(acc[None, :], combine)[0])


def row_terms(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def tree_dot(a, b):
    return tree_sum(row_terms(a, b))


def tree_max(t):
    return tree_sum(t, _larger)


def row_times_matrix(rows, m):
    """(x m_0k + y m_1k) + z m_2k"""
    rows, m = np.asarray(rows, f64), np.asarray(m, f64).reshape(3, 3)
    x, y, z = rows[:, 0:1], rows[:, 1:2], rows[:, 2:3]
    return (x * m[0] + y * m[1]) + z * m[2]


# ------------------------------------------------------------------------------------------------ the four updates
def kicked(v, f, dt, zero_first=False):
    if zero_first:
        v = v * 0.0
    return v + dt * f


def mixed(v, f, a, ff, vv, multiplier=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (1.0 - a) * v + a * f / np.sqrt(ff) * np.sqrt(vv)
    return out if multiplier is None else multiplier * out


def capped(v, dt, maxstep):
    """ABC-FIRE's cap per component — the caller applies it only when no component of v is zero"""
    size = np.abs(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(size * dt > maxstep, (maxstep / dt) * (v / size), v)


def limited(dr, norm, maxstep):
    return maxstep * dr / norm if norm > maxstep else dr


# ------------------------------------------------------------------------------------------------ the module of kernels.fire
def dots(v, f, record):
    f = _np(f)
    terms = row_terms(f, f)
    record[VF] = 0.0 if v is None else tree_dot(_np(v), f)
    record[FF] = tree_sum(terms)
    record[FMAX2] = tree_max(terms)


def kick(v, f, dt, zero_first, record):
    f = _np(f)
    v[...] = kicked(v, f, dt, zero_first)
    record[FF] = tree_dot(f, f)
    record[VV] = tree_dot(v, v)


def mix(v, f, a, abc_multiplier, use_abc, dt, record):
    v[...] = mixed(v, _np(f), a, record[FF], record[VV], abc_multiplier if use_abc else None)
    dr = dt * v
    record[DRDR] = tree_dot(dr, dr)
    record[ZEROS] = tree_sum((v == 0.0).sum(axis=1).astype(f64))


def move(v, dr, n_atoms, scale, dt, maxstep, mode, record, x=None, y=None, z=None, x_out=None, y_out=None, z_out=None, unstrained=None):
    if mode == MOVE_CAP and record[ZEROS] == 0.0:
        v[...] = capped(v, dt, maxstep)
    d = scale * v
    if mode == MOVE_NORM:
        d = limited(d, np.sqrt(record[DRDR]), maxstep)
    dr[...] = d
    if unstrained is not None:
        unstrained[...] = unstrained + d[:n_atoms]
    else:
        for k, (src, out) in enumerate(((x, x_out), (y, y_out), (z, z_out))):
            out[...] = _np(src) + d[:n_atoms, k]


def rowmat(rows, matrix, out_rows=None, out_x=None, out_y=None, out_z=None):
    got = row_times_matrix(_np(rows), matrix)
    if out_rows is not None:
        out_rows[...] = got
    else:
        out_x[...], out_y[...], out_z[...] = got[:, 0], got[:, 1], got[:, 2]


def scatter_rows(rows, perm, out_rows):
    out_rows[np.asarray(_np(perm), np.int64)] = _np(rows)


def total(values, word, record):
    record[word] = tree_sum(_np(values))


# ------------------------------------------------------------------------------------------------ the whole algorithm
def voigt_matrix(s):
    return np.array([[s[0], s[5], s[4]], [s[5], s[1], s[3]], [s[4], s[3], s[2]]])


def run(system, steps, fmax=1e-4, dot=np.vdot, matmul=np.matmul, keep_unstrained=False, state=None, dt=0.1, maxstep=0.2, dtmax=1.0,
        dtmin=2e-3, Nmin=20, finc=1.1, fdec=0.5, astart=0.25, fa=0.99, use_abc=False, optimize_cell=False, mask=None, cell_factor=None,
        hydrostatic_strain=False, constant_volume=False, scalar_pressure=0.0):
    """-> dict(converged, v, dt, a, Nsteps, uphill: the steps that went uphill, faster: the steps that raised dt, steps: how many were evaluated).  ``state``: the dict of
    an earlier run to carry dt, a, Nsteps (and orig_box) on from.  ``dot(a, b)`` is the sum of products over two (n, 3) arrays,
    ``matmul(rows, m)`` the row-times-3x3 product; ``keep_unstrained`` keeps u as the state (u += dr, positions = u (I + deform))
    where the default solves u back from the strained positions in every move"""
    n = system.N
    a, count = astart, 0
    home = system.box.box.copy() if optimize_cell else None
    if state is not None:
        dt, a, count = state["dt"], state["a"], state["Nsteps"]
        home = state.get("orig_box", home)
    if optimize_cell:
        cell_factor = float(n) if cell_factor is None else cell_factor
        mask = np.ones((3, 3)) if mask is None else (voigt_matrix(mask) if len(mask) == 6 else np.asarray(mask))
    eye = np.eye(3)
    kept = {}

    def gradient():
        return np.linalg.solve(home, system.box.box).T

    def forces():
        f = system.get_force()
        if not optimize_cell:
            return f
        volume = system.box.volume
        w = (-voigt_matrix(system.get_stress()) - np.diag([scalar_pressure] * 3)) * volume
        g = gradient()
        w = np.linalg.solve(g, w.T).T
        if hydrostatic_strain:
            w = np.diag([w.trace() / 3.0] * 3)
        if (mask != 1.0).any():
            w *= mask
        if constant_volume:
            t = w.trace()
            np.fill_diagonal(w, np.diag(w) - t / 3.0)
        return np.vstack((matmul(f, g), w / cell_factor))

    def displace(dr):
        frame = system.data
        if optimize_cell:
            g = gradient()
            if keep_unstrained:
                if "u" not in kept:
                    kept["u"] = np.linalg.solve(g, frame.select("x", "y", "z").to_numpy().T).T
                u = kept["u"] = kept["u"] + dr[:n]
            else:
                u = np.linalg.solve(g, frame.select("x", "y", "z").to_numpy().T).T + dr[:n]
            deform = ((g + dr[n:] / cell_factor) - eye).T * mask
            system.update_box(home @ (eye + deform))
            pos = matmul(u, eye + deform)
            new = {c: pos[:, k] for k, c in enumerate("xyz")}
        else:
            new = {c: frame[c].to_numpy() + dr[:, k] for k, c in enumerate("xyz")}
        system.update_data(frame.with_columns(**new), True, True)

    if optimize_cell and keep_unstrained:  # (the state is made before the first force evaluation)
        kept["u"] = np.linalg.solve(gradient(), system.data.select("x", "y", "z").to_numpy().T).T
    v, uphill, faster, done = None, [], [], 0
    out = lambda ok: dict(converged=ok, v=v, dt=dt, a=a, Nsteps=count, uphill=uphill, faster=faster, steps=done, orig_box=home)
    for step in range(steps):
        f = forces()
        done = step + 1
        if np.sqrt((f**2).sum(axis=1).max()) < fmax:
            return out(True)
        if v is None:
            v = np.zeros_like(f)
        elif dot(f, v) > 0.0:
            count += 1
            if count > Nmin:
                faster.append(step)
                dt, a = min(dt * finc, dtmax), a * fa
        else:
            uphill.append(step)
            count, dt, a = 0, max(dt * fdec, dtmin), astart
            displace(-0.5 * dt * v)
            f = forces()
            v = v * 0.0
        v = kicked(v, f, dt)
        if use_abc:
            a = max(a, 1e-10)
            v = mixed(v, f, a, dot(f, f), dot(v, v), 1.0 / (1.0 - (1.0 - a) ** (count + 1)))
            if np.all(v):
                v = capped(v, dt, maxstep)
            dr = dt * v
        else:
            v = mixed(v, f, a, dot(f, f), dot(v, v))
            dr = dt * v
            dr = limited(dr, np.sqrt(dot(dr, dr)), maxstep)
        displace(dr)
    system.calc.results = {}
    return out(False)
