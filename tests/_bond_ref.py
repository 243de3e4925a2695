"""A numpy restatement of the reference's compute_bond / compute_adf (src/bond_analysis.cpp:8-279) for the bond-analysis tests.

Same call signatures as ``mdapy_amd._bond_analysis`` (it can stand in for ``kernels.bond_analysis``).  Every floating-point
expression is the reference's, operation for operation; the angle bin takes ``np.arccos`` for the bulk and redoes with
``math.acos`` (the C library's, like the reference) every triplet within 1e-7 of a bin edge, where the two may disagree.
A triplet whose cosine is NaN (a zero distance) is not counted — the library's defined answer where the reference's is
undefined."""
import math

import numpy as np

PI = 3.14159265358979323846


def _pbc(box, boundary):
    """box.pbc of src/box.h:93-124 over arrays"""
    m = np.asarray(box, dtype=np.float64)[:3].ravel()
    tri = any(abs(m[3 * i + j]) > 1e-10 for i in range(3) for j in range(3) if i != j) or m[0] < 0 or m[4] < 0 or m[8] < 0
    bnd = [int(v) for v in np.asarray(boundary).ravel()]
    if tri:  # box.h:178-203
        det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
        inv_det = 1.0 / det
        hi = [(m[4] * m[8] - m[5] * m[7]) * inv_det, -(m[1] * m[8] - m[2] * m[7]) * inv_det, (m[1] * m[5] - m[2] * m[4]) * inv_det,
              -(m[3] * m[8] - m[5] * m[6]) * inv_det, (m[0] * m[8] - m[2] * m[6]) * inv_det, -(m[0] * m[5] - m[2] * m[3]) * inv_det,
              (m[3] * m[7] - m[4] * m[6]) * inv_det, -(m[0] * m[7] - m[1] * m[6]) * inv_det, (m[0] * m[4] - m[1] * m[3]) * inv_det]

    def apply(dx, dy, dz):
        if tri:
            fx = dx * hi[0] + dy * hi[3] + dz * hi[6]
            fy = dx * hi[1] + dy * hi[4] + dz * hi[7]
            fz = dx * hi[2] + dy * hi[5] + dz * hi[8]
            if bnd[0]:
                fx = fx - np.floor(fx + 0.5)
            if bnd[1]:
                fy = fy - np.floor(fy + 0.5)
            if bnd[2]:
                fz = fz - np.floor(fz + 0.5)
            return (fx * m[0] + fy * m[3] + fz * m[6], fx * m[1] + fy * m[4] + fz * m[7], fx * m[2] + fy * m[5] + fz * m[8])
        out = []
        for k, d in enumerate((dx, dy, dz)):
            L = m[4 * k]
            out.append(d - L * np.floor(d / L + 0.5) if bnd[k] else d)
        return tuple(out)

    return apply


def angle_bins(c, delta_theta, nbin):
    """bin of each cosine (no NaN in c): min(floor(acos(c) * 180 / PI * (1 / delta_theta)), nbin - 1), with the C library's acos
    wherever np.arccos could put it on the other side of an edge"""
    c = np.clip(c, -1.0, 1.0)
    inv = 1.0 / delta_theta
    v = np.arccos(c) * 180.0 / PI * inv
    near = np.abs(v - np.round(v)) < 1e-7
    if near.any():
        exact = np.array([math.acos(t) for t in c[near].tolist()], dtype=np.float64)
        v[near] = exact * 180.0 / PI * inv
    b = np.floor(v)
    return np.minimum(b, nbin - 1).astype(np.int64)


def _np(a):
    return np.asarray(a.to_numpy() if hasattr(a, "to_numpy") else a)


def _rows(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number):
    x, y, z = (np.asarray(_np(a), np.float64) for a in (x, y, z))
    v, d = np.asarray(_np(verlet_list), np.int64), np.asarray(_np(distance_list), np.float64)
    nn = np.clip(np.asarray(_np(neighbor_number), np.int64), 0, v.shape[1])
    return x, y, z, v, d, nn, _pbc(box, boundary)


def _vectors(x, y, z, v, pbc, col):
    i = np.arange(v.shape[0])
    j = np.where((v[:, col] >= 0) & (v[:, col] < len(x)), v[:, col], i)
    return pbc(x[j] - x[i], y[j] - y[i], z[j] - z[i])


def _pairs(v, nn):
    for jj in range(v.shape[1]):
        for kk in range(jj + 1, v.shape[1]):
            rows = np.nonzero(kk < nn)[0]
            if rows.size:
                yield jj, kk, rows


def compute_bond(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, bond_length_distribution,
                 bond_angle_distribution, delta_r, delta_theta, rc, nbins, num_t=1):
    x, y, z, v, d, nn, pbc = _rows(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number)
    N, M = v.shape
    i = np.arange(N)[:, None]
    ok = (np.arange(M)[None, :] < nn[:, None]) & (v > i) & (d <= rc)
    b = np.floor(d[ok] * (1.0 / delta_r))
    b = np.minimum(b, nbins - 1).astype(np.int64)
    bond_length_distribution += np.bincount(b, minlength=nbins)[:nbins].astype(bond_length_distribution.dtype)
    vec = [_vectors(x, y, z, v, pbc, col) for col in range(M)]
    hist = np.zeros(nbins, np.int64)
    for jj, kk, rows in _pairs(v, nn):
        rp, rq = d[rows, jj], d[rows, kk]
        keep = (rp <= rc) & (rq <= rc)
        rows, rp, rq = rows[keep], rp[keep], rq[keep]
        if not rows.size:
            continue
        (px, py, pz), (qx, qy, qz) = ((a[rows] for a in vec[jj]), (a[rows] for a in vec[kk]))
        with np.errstate(invalid="ignore", divide="ignore"):
            c = (px * qx + py * qy + pz * qz) / (rp * rq)
        c = c[~np.isnan(c)]
        hist += np.bincount(angle_bins(c, delta_theta, nbins), minlength=nbins)
    bond_angle_distribution += hist.astype(bond_angle_distribution.dtype)


def compute_adf(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, delta_theta, rc_list, pair_list,
                type_list, nbins, bond_angle_distribution, num_t=1):
    x, y, z, v, d, nn, pbc = _rows(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number)
    N, M = v.shape
    t = np.asarray(_np(type_list), np.int64)
    pats = np.asarray(pair_list, np.int64).reshape(-1, 3)
    rng = np.asarray(rc_list, np.float64).reshape(-1, 4)
    vec = [_vectors(x, y, z, v, pbc, col) for col in range(M)]
    tj = np.where((v >= 0) & (v < N), v, np.arange(N)[:, None])
    tj = t[tj]
    ti = t
    hist = np.zeros((pats.shape[0], nbins), np.int64)
    for jj, kk, rows in _pairs(v, nn):
        rp, rq = d[rows, jj], d[rows, kk]
        (px, py, pz), (qx, qy, qz) = ((a[rows] for a in vec[jj]), (a[rows] for a in vec[kk]))
        with np.errstate(invalid="ignore", divide="ignore"):
            c = (px * qx + py * qy + pz * qz) / (rp * rq)
        good = ~np.isnan(c)
        bins = np.zeros(len(c), np.int64)
        bins[good] = angle_bins(c[good], delta_theta, nbins)
        a, tp, tq = ti[rows], tj[rows, jj], tj[rows, kk]
        for m, (A, B, C) in enumerate(pats):
            lo1, hi1, lo2, hi2 = rng[m]
            jp = (tp == B) & (rp <= hi1) & (rp >= lo1)
            kq = (tq == C) & (rq <= hi2) & (rq >= lo2)
            hit = (a == A) & good & jp & kq
            if B != C:
                jq = (tq == B) & (rq <= hi1) & (rq >= lo1)
                kp = (tp == C) & (rp <= hi2) & (rp >= lo2)
                hit2 = (a == A) & good & jq & kp
                hist[m] += np.bincount(bins[hit2], minlength=nbins)
            hist[m] += np.bincount(bins[hit], minlength=nbins)
    bond_angle_distribution += hist.reshape(bond_angle_distribution.shape).astype(bond_angle_distribution.dtype)
