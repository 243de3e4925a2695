"""mdapy_amd — MI355X-native (gfx950, hand-written HIP) implementation of mdapy's
neighbor-list + per-atom structural-analysis hot path, behind mdapy's own
``System`` / ``cal_*`` / ``_module.function`` API.  See DESIGN.md."""
__version__ = "0.1.0"

from .box import Box
from .frame import Frame
from .system import System
from .neighbor import Neighbor
from .knn import NearestNeighbor
from .common_neighbor_analysis import CommonNeighborAnalysis
from .centro_symmetry_parameter import CentroSymmetryParameter
from .identify_diamond_structure import IdentifyDiamondStructure
from .steinhardt_bond_orientation import SteinhardtBondOrientation
from .polyhedral_template_matching import PolyhedralTemplateMatching
from .radial_distribution_function import RadialDistributionFunction
from .warren_cowley_parameter import WarrenCowleyParameter
from .atomic_strain import AtomicStrain
from .calculator import CalculatorMP
from .eam import EAM
from .nep import NEP, QNEP
from . import minimizer
from .minimizer import FIRE
from .chill_plus import ChillPlus
from .wigner_seitz_defect import WignerSeitzAnalysis
from .lindemann_parameter import LindemannParameter
from .mean_squared_displacement import MeanSquaredDisplacement
from .void_analysis import VoidAnalysis
from .trajectory import Trajectory
from .unwrap_trajectory import unwrap_trajectory
from .vdw_radii import VDW_RADII, vdw_radius
from .build_lattice import build_crystal, build_hea, build_hea_fromsystem
from .sqs import SQS
from .create_polycrystal import CreatePolycrystal
from .parallel import get_num_threads

__all__ = [
    "Box", "Frame", "System", "Neighbor", "NearestNeighbor", "CommonNeighborAnalysis", "CentroSymmetryParameter",
    "IdentifyDiamondStructure", "SteinhardtBondOrientation", "PolyhedralTemplateMatching", "RadialDistributionFunction", "WarrenCowleyParameter",
    "AtomicStrain", "CalculatorMP", "EAM", "NEP", "QNEP", "FIRE", "ChillPlus", "WignerSeitzAnalysis", "LindemannParameter", "MeanSquaredDisplacement", "VoidAnalysis",
    "Trajectory", "unwrap_trajectory", "VDW_RADII", "vdw_radius",
    "build_crystal", "build_hea", "build_hea_fromsystem", "SQS", "CreatePolycrystal", "get_num_threads",
]
