"""MI355X-native evaluator for the IE-ACHE Cloud path (Cloud/cloud.c + libtfhe
gate bootstrapping).  The product is the HIP shared library `libieache.so`
(C ABI: include/ieache.h); this package is the thin ctypes host side mirroring
the reference's Python caller (Cloud/dragonfly_cipher_cloud.py:1219-1327).
"""
from .evaluator import (  # noqa: F401
    CIRC_ADD, CIRC_SUB, CIRC_RSUB, CIRC_MUL, CIRC_MULADD, CIRC_ADD_KS, CIRC_SUB_KS, CIRC_RSUB_KS, CIRC_MUL_WALLACE,
    GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_MUX, circ_chain,
    GATE_NOR, GATE_XNOR, GATE_ANDNY, GATE_ANDYN, GATE_ORNY, GATE_ORYN, GATE_TYPES, FALSE, TRUE, NOT, Netlist, CompiledNetlist,
    CircuitInfo, Context, IeacheError, Params, Stats, build_library, circuit_info, circuit_level_cap, circuit_simulate,
    default_params, device_count, debug_forward_path, lib, library_path,
    GATE_MAJ3, GATE_XOR3, CIRC_ADD_FA, CIRC_SUB_FA, CIRC_RSUB_FA, CIRC_MUL_FA, circuit_gate_count,
    PBS_NO_KEYSWITCH, PBS_TLWE_POLYS, PBS_ACCUMULATOR, PBS_MULTI_MAX_FACTORS, Group, GROUP_MAX_DEVICES, Job,
    TgswSet, Automaton, AUTOMATON_MAX_STATES, AUTOMATON_MAX_STEPS, automaton_tables, LUT_TREE_MAX_DEPTH, ROTATE_MAX_STEPS, LUT_READ_NO_KEYSWITCH,
    UNPACK_NO_KEYSWITCH, ROWS_LWE, ROWS_EXTRACTED, ROWS_TLWE, LINEAR_MAX_DIM,
    FFT_FORWARD_FORMS, FFT_INVERSE_FORMS, FFT_PAIRED_FORMS, TWIDDLE_ENTRIES,
)
from . import tools  # noqa: F401
from . import netlists  # noqa: F401
from . import automata  # noqa: F401
from . import layers  # noqa: F401
from . import programs  # noqa: F401
from .programs import WordProgram, Register, netlist_export  # noqa: F401
from .programs import FAMILY_REFERENCE, FAMILY_KOGGE_STONE, FAMILY_CARRY_SAVE, FAMILY_FULL_ADDER  # noqa: F401
from .compute import compute, compute_final, FAILURE_SIZE  # noqa: F401
