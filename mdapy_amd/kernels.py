"""The one door between the host layer and the C ABI.

Every analysis class reaches libmdapy_amd.so through the attributes of this module — one shim module per nanobind
extension of the reference (``mdapy._neighbor`` ... ``mdapy._repeat_cell``, CMakeLists.txt:71-100; same function names and
argument order, implemented by ctypes calls into include/mdapy_amd.h).  Keeping the door in one place is what lets the
CPU test-suite swap the shims for the oracle without a backend switch inside the package."""
from . import _aja as aja
from . import _atomtemp as atomtemp
# (not in NAMES: the CPU suite's oracle backend asserts an adapter for every name there, and the oracle has no bond analysis;
# its tests install a restatement of their own as kernels.bond_analysis — one by one, or all of them with
# tests/_oracle_backend.py's install_consumers, as the randomised sweeps do)
from . import _bond_analysis as bond_analysis
# (not in NAMES either: the oracle has no adapter for the bond pairs and the molecule compositions; their tests install a
# restatement as kernels.build_bond)
from . import _build_bond as build_bond
# (not in NAMES either: the oracle has no CHILL+; its tests install a restatement as kernels.chill_plus)
from . import _chill_plus as chill_plus
from . import _cluster as cluster
from . import _cna as cna
from . import _cnp as cnp
from . import _csp as csp
# (not in NAMES either: the oracle has no EAM; its tests install a restatement as kernels.eam)
from . import _eam as eam
from . import _fast_knn as fast_knn
# (not in NAMES either: the oracle has no minimizer; its tests install a restatement as kernels.fire)
from . import _fire as fire
from . import _fccpft as fccpft
# (not in NAMES either: the oracle has no Lindemann index; its tests install a restatement as kernels.lindemann)
from . import _lindemann as lindemann
# (not in NAMES either: neither the reference nor the oracle has a compiled MSD; its tests install a restatement as kernels.msd)
from . import _msd as msd
# (not in NAMES either: the oracle has no NEP; its tests install a restatement as kernels.nep)
from . import _nep as nep
from . import _neighbor as neighbor
from . import _order as order
from . import _polycrystal as polycrystal
from . import _ptm as ptm
from . import _rdf as rdf
from . import _repeat_cell as repeat_cell
# (not in NAMES either: the reference's farthest-point sampling and PCA are numpy, the oracle has neither; their tests install a
# restatement as kernels.sample)
from . import _sample as sample
from . import _sbo as sbo
from . import _sfc as sfc
# (not in NAMES either: the oracle has no SQS engine; its tests install a restatement as kernels.sqs)
from . import _sqs as sqs
# (not in NAMES either: the oracle has no atomic strain; its tests install a restatement as kernels.strain)
from . import _strain as strain
from . import _structure_entropy as structure_entropy
# (not in NAMES either: the oracle has no tokenizer or formatter; the readers and writers of load_save check both against Python's
# own float() and format())
from . import _text as text
# (not in NAMES either: neither the reference nor the oracle has a compiled unwrap; its tests install a restatement as kernels.unwrap)
from . import _unwrap as unwrap
# (not in NAMES either: the oracle has no adapter for the void analysis; its tests install a restatement as kernels.void and as
# kernels.neighbor._fill_cell_for_void)
from . import _void as void
from . import _voronoi as voronoi
from . import _wcp as wcp

NAMES = ("aja", "atomtemp", "cluster", "cna", "cnp", "csp", "fast_knn", "fccpft", "neighbor", "order", "polycrystal", "ptm", "rdf",
         "repeat_cell", "sbo", "sfc", "structure_entropy", "voronoi", "wcp")
