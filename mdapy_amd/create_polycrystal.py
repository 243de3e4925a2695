"""Polycrystal builder — the drop-in for ``mdapy.create_polycrystal.CreatePolycrystal``
(src/mdapy/create_polycrystal.py:20-850), metallic grains with optional graphene at the grain boundaries.

Recipe: Voronoi tessellation of the seed points (periodic box); every cell is filled with a rotated copy of the unit
cell's lattice, cut at the cell's faces; atoms of neighbouring grains that end up closer than ``metal_overlap_dis`` are
thinned out; everything is wrapped into the box.  With ``add_graphene`` a honeycomb sheet is laid on every cell face
larger than ``face_threshold`` and the metal / carbon contacts are thinned by their own distances.

Where the work is done: the cells — :class:`mdapy_amd.voronoi.Container` (csrc/voronoi.hip); filling a grain —
``transform_and_filter`` (csrc/polycrystal.hip: rotate, translate, half-space test against the face planes in LDS,
order-preserving compaction); contacts — ``filter_overlap_atom[_with_grain]`` (csrc/rows.hip, csrc/polycrystal.hip;
the reference's order-dependent sweep in its serial order); wrapping — ``System.wrap_pos``.  The random draws (seed
positions, Euler angles) are made in the reference's order from the same generator, so a given ``randomseed`` gives the
same grains."""
import numpy as np

from . import geometry, kernels, policy
from .box import Box
from .frame import Frame
from .parallel import get_num_threads
from .voronoi import Container

_CC_BOND = 1.42          # A, graphene
_CC_CONTACT = 1.4        # A: carbon atoms of different sheets closer than this are thinned
_METAL_CONTACT = 2.0     # A: default metal-metal contact distance when graphene is added


def _given_or_drawn(given, shape, draw, what):
    if given is None:
        return draw()
    given = np.asarray(given, float)
    if given.shape != shape:
        raise ValueError(f"{what} shape must be ({shape[0]}, 3), got {given.shape}")
    return given


class CreatePolycrystal:
    def __init__(self, unitcell, box, seed_number, seed_position=None, theta_list=None, randomseed=None,
                 metal_overlap_dis=None, add_graphene=False, metal_gra_overlap_dis=3.0, face_threshold=0.0,
                 need_rotation=True):
        self.unitcell, self.box = unitcell, Box(box)
        if int(np.sum(self.box.boundary)) != 3:
            raise ValueError("Free boundary condition is not supported.")
        if self.box.triclinic:
            raise ValueError("Triclinic box is not supported")
        self.seed_number = int(seed_number)
        self.metal_overlap_dis, self.metal_gra_overlap_dis = metal_overlap_dis, metal_gra_overlap_dis
        self.add_graphene, self.need_rotation, self.face_threshold = bool(add_graphene), need_rotation, face_threshold
        self.randomseed = int(np.random.randint(0, 1_000_000_000) if randomseed is None else randomseed)
        self.rng = np.random.default_rng(self.randomseed)
        wanted = (self.seed_number, 3)
        # (positions are drawn before angles: the order fixes what a given randomseed produces)
        self.seed_position = _given_or_drawn(seed_position, wanted, lambda: self.rng.random(wanted) * np.diag(self.box.box),
                                             "seed_position")
        self.theta_list = _given_or_drawn(theta_list, wanted, lambda: self.rng.uniform(-180, 180, wanted), "theta_list")

    # names of the reference class' helpers, kept for its users
    _get_rotation_matrix = staticmethod(lambda theta_deg, axis_tuple: geometry.rotation_about(axis_tuple, theta_deg))
    _get_plane_equation_coeffs_for_cell = staticmethod(geometry.inward_planes)
    _points_in_polygon_2d = staticmethod(geometry.inside_polygon)

    def _graphene_on_faces(self, cell, sheet, planes):
        """carbon atoms on the faces of one cell: the sheet turned onto each face's normal, centred on the face, cut to it"""
        pieces = []
        for f, plane in enumerate(planes):
            if cell.face_areas[f] <= self.face_threshold:
                continue
            corners = cell.vertices[cell.face_vertices[f]]
            normal = plane[:3] / np.linalg.norm(plane[:3])
            turned = sheet @ geometry.rotation_taking(np.array([0.0, 0.0, 1.0]), normal).T
            placed = turned - turned.mean(axis=0) + corners.mean(axis=0)
            cut = geometry.on_face(placed, corners, normal)
            if len(cut):
                pieces.append(cut)
        if not pieces:
            raise AssertionError("No graphene atoms generated")
        return np.vstack(pieces)

    def _lattice_block(self, reach):
        """positions of enough copies of the unit cell to cover a sphere of radius ``reach``, and their centroid"""
        copies = np.ceil(reach / self.unitcell.box.get_thickness()).astype(int)
        block, _ = policy.replica(self.unitcell.data, self.unitcell.box, copies, all_columns=False)
        xyz = tuple(np.ascontiguousarray(block[c].to_numpy(), dtype=np.float64) for c in ("x", "y", "z"))
        return xyz, np.array([axis.mean() for axis in xyz])

    def _graphene_sheet(self, reach):
        """a flat honeycomb sheet at least 2 * reach wide: covers any face once it is centred on it"""
        from .build_lattice import lattice_positions

        a = _CC_BOND * 3 ** 0.5
        width = 2.0 * reach
        return lattice_positions("graphene", a, int(np.ceil(width / a)), int(np.ceil(width / (a * 3 ** 0.5 / 2.0))), 1, c=1.0)[0]

    def _get_pos(self):
        """-> positions, grain ids (1-based), types (1 metal, 2 carbon) of everything generated, grain by grain"""
        reach = max(cell.cavity_radius for cell in self.con)
        lattice, centre = self._lattice_block(reach)
        sheet = self._graphene_sheet(reach) if self.add_graphene else None
        positions, grains, kinds = [], [], []
        for n, cell in enumerate(self.con):
            turn = geometry.euler_xyz(self.theta_list[n]) if self.need_rotation else geometry.rotation_about((1.0, 0.0, 0.0), 0)
            planes = geometry.inward_planes(cell)
            metal = kernels.polycrystal.transform_and_filter(*lattice, turn, centre, cell.pos, planes, get_num_threads())
            positions.append(metal)
            kinds.append(np.ones(len(metal), np.int32))
            members = len(metal)
            if sheet is not None:
                carbon = self._graphene_on_faces(cell, sheet, planes)
                positions.append(carbon)
                kinds.append(np.full(len(carbon), 2, np.int32))
                members += len(carbon)
            grains.append(np.full(members, n + 1, np.int32))
        return np.vstack(positions), np.concatenate(grains), np.concatenate(kinds)

    def _contacts_kept(self, x, y, z, kinds, grains):
        """mask of the atoms that survive the thinning of too-close contacts (None: nothing to thin)"""
        where = tuple(np.ascontiguousarray(c) for c in (x, y, z))
        if self.add_graphene:
            metal = _METAL_CONTACT if self.metal_overlap_dis is None else float(self.metal_overlap_dis)
            kept = kernels.neighbor.filter_overlap_atom_with_grain(*where, kinds, grains, *policy.box_args(self.box), metal,
                                                                   _CC_CONTACT, float(self.metal_gra_overlap_dis),
                                                                   get_num_threads())
        elif self.metal_overlap_dis is not None:
            kept = kernels.neighbor.filter_overlap_atom(*where, *policy.box_args(self.box), float(self.metal_overlap_dis),
                                                        get_num_threads())
        else:
            return None
        return np.asarray(kept, bool)

    def compute(self, verbose=True):
        """-> System with columns (element,) x, y, z, grain_id, type"""
        from .system import System

        self.con = Container(np.ascontiguousarray(self.seed_position, dtype=np.float64), Box(self.box.box))
        self.volume = np.array([cell.volume for cell in self.con])
        if verbose:
            print(f"  Number of grains: {self.seed_number}\n  Average volume:   {self.volume.mean():>10.2f} A^3")
        pos, grains, kinds = self._get_pos()
        generated = len(pos)
        shift = self.box.origin.copy()
        x, y, z = (pos[:, a] + shift[a] for a in range(3))
        kept = self._contacts_kept(x, y, z, kinds, grains)
        if kept is not None:
            x, y, z, grains, kinds = (c[kept] for c in (x, y, z, grains, kinds))
        if verbose:
            print(f"  Total atoms generated: {generated:,}; removed: {generated - len(x):,}")
        columns = {"x": x, "y": y, "z": z, "grain_id": grains, "type": kinds}
        if "element" in self.unitcell.data.columns:  # type 1 carries the unit cell's element, type 2 is carbon
            metal_name = self.unitcell.data["element"].to_numpy()[0]
            columns = {"element": np.where(kinds == 2, "C", metal_name), **columns}
        built = System(data=Frame(columns), box=self.box)
        built.wrap_pos()
        return built
