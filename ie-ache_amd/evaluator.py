"""ctypes binding of libieache.so (include/ieache.h).

There is no CPU fallback: if the HIP library is missing this module raises on
first use, and every evaluation entry point needs a GPU.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = None

CIRC_ADD, CIRC_SUB, CIRC_RSUB, CIRC_MUL, CIRC_MULADD = 1, 2, 3, 4, 5
CIRC_ADD_KS, CIRC_SUB_KS, CIRC_RSUB_KS = 6, 7, 8  # Kogge-Stone variants (decrypt-identical, not bit-identical)
CIRC_MUL_WALLACE = 9  # carry-save multiplier (decrypt-identical, not bit-identical)
GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_MUX = 0, 1, 2, 3, 4
GATE_NOR, GATE_XNOR, GATE_ANDNY, GATE_ANDYN, GATE_ORNY, GATE_ORYN = 5, 6, 7, 8, 9, 10  # libtfhe boot-gates.cpp
GATE_TYPES = 11
LUT_TREE_MAX_DEPTH = 12  # IEACHE_LUT_TREE_MAX_DEPTH
ROTATE_MAX_STEPS = 64  # IEACHE_ROTATE_MAX_STEPS
LUT_READ_NO_KEYSWITCH = 1  # flag of ieache_lut_read*: the extracted rows are the result
UNPACK_NO_KEYSWITCH = 1  # the same for ieache_unpack* and ieache_word_read*
PBS_MULTI_MAX_FACTORS = 64  # most factor polynomials of one ieache_pbs_multi* call
PBS_NO_KEYSWITCH = 1  # flag of ieache_pbs*: the extracted samples are the result (tfhe_bootstrap_woKS_FFT)
PBS_TLWE_POLYS = 4    # ... the table is [n_polys][2][N]: TLWE samples under the ring key (an encrypted table)
PBS_ACCUMULATOR = 8   # ... of ieache_pbs only: the whole rotated accumulators [2][N] are the result (tfhe_blindRotate_FFT)
GATE_MAJ3, GATE_XOR3 = 32, 33  # three-input gates of one bootstrap each (codes outside 0 .. GATE_TYPES-1: include/ieache.h)
CIRC_ADD_FA, CIRC_SUB_FA, CIRC_RSUB_FA, CIRC_MUL_FA = 16, 17, 18, 19  # on the MAJ3 / XOR3 full adder (decrypt-identical)
GROUP_MAX_DEVICES = 16  # most members of a device group (IEACHE_GROUP_MAX_DEVICES)
# references inside a Netlist (IEACHE_NET_*): wire << 1 | negated, or a constant
FALSE, TRUE = -2, -1


def NOT(ref):
    """bootsNOT of a netlist reference (free: a sign flag, no bootstrap)."""
    return int(ref) ^ 1


def circ_chain(k1, k2, flip=True):
    """IEACHE_CIRC_CHAIN: stage 1 = k1(A, B), stage 2 = k2(answer, C) (flip) or k2(C, answer) --
    compute() followed by compute_final() (Cloud/dragonfly_cipher_cloud.py:1219-1327) as one DAG."""
    assert 1 <= k1 <= 4 and 1 <= k2 <= 4
    return 32 + (k1 - 1) + 4 * (k2 - 1) + (0 if flip else 16)


class IeacheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ieache error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("n", "N", "k", "l", "Bgbit", "ks_t", "ks_basebit")] + \
               [(f, C.c_double) for f in ("lwe_alpha_min", "lwe_alpha_max", "tlwe_alpha_min", "tlwe_alpha_max")]

    @property
    def bk_count(self):
        return self.n * (self.k + 1) * self.l * (self.k + 1) * self.N

    @property
    def ksk_count(self):
        return self.k * self.N * self.ks_t * (1 << self.ks_basebit) * (self.n + 1)

    @property
    def lwe_stride(self):
        return (self.n + 1 + 3) & ~3

    def copy(self, **kw):
        p = Params.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class Stats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("blind_rotate_ms", C.c_double), ("keyswitch_ms", C.c_double),
                ("blind_rotate_launches", C.c_int64), ("keyswitch_launches", C.c_int64),
                ("bootstraps", C.c_int64), ("levels", C.c_int64), ("chunks", C.c_int64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class Job(C.Structure):
    """ieache_job: one circuit's batch of a joint call (Context.eval_jobs builds these)."""
    _fields_ = [("kind", C.c_int), ("bits", C.c_int), ("netlist", C.c_void_p), ("batch", C.c_size_t),
                ("in_lwe", C.c_void_p), ("out_lwe", C.c_void_p)]


class CircuitInfo(C.Structure):
    _fields_ = [("n_inputs", C.c_int32), ("n_outputs", C.c_int32), ("n_slots", C.c_int32), ("depth", C.c_int32),
                ("max_width", C.c_int32), ("bootstraps", C.c_int64), ("n_and", C.c_int64), ("n_xor", C.c_int64),
                ("sched_max_width", C.c_int32), ("folded", C.c_int32), ("reference_bootstraps", C.c_int64),
                ("sched_levels", C.c_int32), ("level_cap", C.c_int32)]


def library_path():
    # IEACHE_LIBRARY: another build of the same library (A/B of compiler flags: scripts/build_alt.sh)
    return os.environ.get("IEACHE_LIBRARY") or os.path.join(_PKG, "libieache.so")


def build_library(jobs=4):
    """Compile libieache.so and the `cloud` shim for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_PKG, "csrc")])


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise IeacheError(-19, "HIP extension %s is missing: run __graft_entry__.build() "
                               "(make -C ie-ache_amd/csrc); there is no CPU fallback" % path)
    # PyTorch bundles its own HIP runtime under the same SONAME (libamdhip64.so.7) as
    # /opt/rocm's.  Two HIP runtimes in one process cannot both own the GPU, so when
    # torch is installed let it load first: the dynamic loader then binds libieache.so
    # to the runtime already in the process.  (The standalone `cloud` executable has
    # no torch in-process and uses /opt/rocm's.)
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    i32p, u32p, u8p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_void_p
    pp, sp = C.POINTER(Params), C.POINTER(Stats)
    L.ieache_version.restype = C.c_char_p
    L.ieache_last_error.restype = C.c_char_p
    L.ieache_last_key_layout.restype = C.c_char_p
    L.ieache_default_params.argtypes = [pp]
    L.ieache_cloud_run.argtypes = [C.c_char_p]
    L.ieache_ctx_create.restype = vp
    L.ieache_ctx_create.argtypes = [C.c_char_p, C.c_int]
    L.ieache_ctx_create_raw.restype = vp
    L.ieache_ctx_create_raw.argtypes = [pp, i32p, i32p, C.c_int]
    L.ieache_ctx_create_device.restype = vp
    L.ieache_ctx_create_device.argtypes = [pp, vp, vp, C.c_int]
    L.ieache_ctx_destroy.argtypes = [vp]
    L.ieache_ctx_params.argtypes = [vp, pp]
    L.ieache_lwe_stride.argtypes = [vp]
    L.ieache_ctx_stream.restype = vp
    L.ieache_ctx_stream.argtypes = [vp]
    L.ieache_ctx_cloud_run.argtypes = [vp, C.c_char_p]
    L.ieache_ctx_set_chunk.argtypes = [vp, C.c_int64]
    L.ieache_ctx_force_generic.argtypes = [vp, C.c_int]
    L.ieache_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.ieache_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.ieache_ctx_fft_guard.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.ieache_ctx_fft_audit.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ieache_ctx_kernel_variant.restype = C.c_char_p
    L.ieache_ctx_kernel_variant.argtypes = [vp]
    L.ieache_ctx_kernel_for_launch.restype = C.c_char_p
    L.ieache_ctx_kernel_for_launch.argtypes = [vp, C.c_int64]
    L.ieache_circuit_info_get.argtypes = [C.c_int, C.c_int, C.POINTER(CircuitInfo)]
    L.ieache_circuit_info_get_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(CircuitInfo)]
    L.ieache_circuit_level_cap.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int]
    L.ieache_ctx_circuit_level_cap.argtypes = [vp, C.c_int, C.c_int, C.c_int64]
    L.ieache_circuit_info_get_cap.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CircuitInfo)]
    L.ieache_circuit_simulate_cap.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p]
    L.ieache_circuit_simulate.argtypes = [C.c_int, C.c_int, u8p, u8p]
    L.ieache_circuit_simulate_ex.argtypes = [C.c_int, C.c_int, C.c_int, u8p, u8p]
    L.ieache_ctx_wait_stream.argtypes = [vp, vp]
    L.ieache_mux_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, sp]
    L.ieache_mux.argtypes = [vp, C.c_size_t, i32p, i32p, i32p, i32p, sp]
    L.ieache_eval_batch.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, i32p, i32p, sp]
    L.ieache_eval_batch_device.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, vp, sp]
    L.ieache_prepare_batch.argtypes = [vp, C.c_int, C.c_int, C.c_size_t]
    L.ieache_gates_device.argtypes = [vp, C.c_int, C.c_size_t, vp, vp, vp, sp]
    L.ieache_gates.argtypes = [vp, C.c_int, C.c_size_t, i32p, i32p, i32p, sp]
    L.ieache_gates3_device.argtypes = [vp, C.c_int, C.c_size_t, vp, vp, vp, vp, sp]
    L.ieache_gates3.argtypes = [vp, C.c_int, C.c_size_t, i32p, i32p, i32p, i32p, sp]
    L.ieache_pbs_device.argtypes = [vp, C.c_size_t, vp, vp, C.c_int32, vp, vp, C.c_int, sp]
    L.ieache_pbs.argtypes = [vp, C.c_size_t, i32p, i32p, C.c_int32, i32p, i32p, C.c_int, sp]
    L.ieache_pbs_multi_device.argtypes = [vp, C.c_size_t, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int, sp]
    L.ieache_pbs_multi.argtypes = [vp, C.c_size_t, i32p, i32p, C.c_int32, i32p, i32p, C.c_int32, i32p, i32p, C.c_int, sp]
    L.ieache_keyswitch_device.argtypes = [vp, C.c_size_t, vp, vp, sp]
    L.ieache_keyswitch.argtypes = [vp, C.c_size_t, i32p, i32p, sp]
    L.ieache_ctx_set_packing_key.argtypes = [vp, C.c_int32, C.c_int32, i32p]
    L.ieache_debug_pack_plan.argtypes = [vp, C.c_size_t, C.c_int32, C.POINTER(C.c_int64)]
    L.ieache_pack_device.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, vp, vp, sp]
    L.ieache_pack.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, sp]
    L.ieache_packing_keygen.argtypes = [pp, i32p, i32p, C.c_int32, C.c_int32, C.c_double, C.c_uint64, i32p]
    L.ieache_pack_reference.argtypes = [pp, C.c_int32, C.c_int32, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, i32p]
    L.ieache_tgsw_prepare.restype = vp
    L.ieache_tgsw_prepare.argtypes = [vp, i32p, C.c_size_t]
    L.ieache_tgsw_prepare_device.restype = vp
    L.ieache_tgsw_prepare_device.argtypes = [vp, vp, C.c_size_t]
    L.ieache_tgsw_prepare_gadget.restype = vp
    L.ieache_tgsw_prepare_gadget.argtypes = [vp, i32p, C.c_size_t, C.c_int32, C.c_int32]
    L.ieache_tgsw_prepare_gadget_device.restype = vp
    L.ieache_tgsw_prepare_gadget_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32]
    L.ieache_tgsw_gadget.argtypes = [vp, i32p, i32p]
    L.ieache_lut_write.argtypes = [vp, vp, C.c_size_t, C.c_int32, i32p, i32p, i32p, i32p, sp]
    L.ieache_lut_write_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, vp, sp]
    L.ieache_tgsw_free.restype = None
    L.ieache_tgsw_free.argtypes = [vp]
    L.ieache_cmux.argtypes = [vp, vp, C.c_size_t, i32p, i32p, i32p, i32p, sp]
    L.ieache_cmux_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, sp]
    L.ieache_lut_tree.argtypes = [vp, vp, C.c_size_t, C.c_int32, i32p, i32p, C.c_int32, i32p, i32p, sp]
    L.ieache_lut_tree_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, C.c_int32, vp, vp, sp]
    L.ieache_lut_scatter.argtypes = [vp, vp, C.c_size_t, C.c_int32, i32p, i32p, i32p, i32p, sp]
    L.ieache_lut_scatter_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, vp, sp]
    L.ieache_lut_scatter_reference.argtypes = [pp, i32p, C.c_size_t, C.c_size_t, C.c_int32, i32p, i32p, i32p, i32p]
    L.ieache_tlwe_rotate.argtypes = [vp, vp, C.c_size_t, C.c_int32, i32p, i32p, i32p, i32p, sp]
    L.ieache_tlwe_rotate_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, vp, sp]
    L.ieache_tlwe_rotate_reference.argtypes = [pp, i32p, C.c_size_t, C.c_size_t, C.c_int32, i32p, i32p, i32p, i32p]
    L.ieache_lut_read.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, i32p, C.c_int32, C.c_int, i32p, sp]
    L.ieache_lut_read_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int, vp, sp]
    L.ieache_lut_read_reference.argtypes = [pp, i32p, C.c_size_t, i32p, C.c_size_t, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, i32p,
                                            C.c_int32, C.c_int, i32p]
    L.ieache_lut_add.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, C.c_int32, i32p, i32p, sp]
    L.ieache_lut_add_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, sp]
    L.ieache_lut_add_reference.argtypes = [pp, i32p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, C.c_int32, i32p, i32p]
    L.ieache_ctx_set_projection_key.argtypes = [vp, C.c_int32, C.c_int32, i32p]
    L.ieache_debug_project_plan.argtypes = [vp, C.c_size_t, C.c_int32, C.POINTER(C.c_int64)]
    L.ieache_tlwe_project.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, sp]
    L.ieache_tlwe_project_device.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, vp, vp, sp]
    L.ieache_tlwe_project_reference.argtypes = [pp, C.c_int32, C.c_int32, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, i32p]
    L.ieache_lut_write_coef.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, sp]
    L.ieache_lut_write_coef_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, sp]
    L.ieache_lut_write_coef_reference.argtypes = [pp, i32p, C.c_size_t, C.c_int32, C.c_int32, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, i32p, i32p, i32p, i32p]
    L.ieache_unpack.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, C.c_int, i32p, sp]
    L.ieache_unpack_device.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int, vp, sp]
    L.ieache_unpack_reference.argtypes = [pp, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, C.c_int, i32p]
    L.ieache_word_read.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, C.c_int32, i32p, C.c_int, i32p, sp]
    L.ieache_word_read_device.argtypes = [vp, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int, vp, sp]
    L.ieache_word_read_reference.argtypes = [pp, i32p, C.c_size_t, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, C.c_int32,
                                             i32p, C.c_int, i32p]
    L.ieache_automaton_create.restype = vp
    L.ieache_automaton_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, i32p, i32p]
    L.ieache_automaton_free.restype = None
    L.ieache_automaton_free.argtypes = [vp]
    L.ieache_automaton_info.argtypes = [vp, i32p, i32p, i32p, C.POINTER(C.c_int64)]
    L.ieache_automaton_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32p, i32p]
    L.ieache_automaton_run.argtypes = [vp, vp, vp, C.c_size_t, i32p, i32p, C.c_int32, i32p, i32p, sp]
    L.ieache_automaton_run_device.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_int32, vp, vp, sp]
    L.ieache_automaton_reference.argtypes = [pp, i32p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, C.c_size_t, i32p, i32p, C.c_int32,
                                             i32p, i32p]
    L.ieache_debug_automaton_plan.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int64)]
    L.ieache_tlwe_extract.argtypes = [vp, C.c_size_t, i32p, i32p, i32p, sp]
    i8p = C.POINTER(C.c_int8)
    L.ieache_lwe_linear_device.argtypes = [vp, C.c_int, C.c_size_t, C.c_int32, C.c_int32, vp, vp, vp, vp, sp]
    L.ieache_lwe_linear.argtypes = [vp, C.c_int, C.c_size_t, C.c_int32, C.c_int32, i8p, i32p, i32p, i32p, sp]
    L.ieache_lwe_linear_reference.argtypes = [pp, C.c_int, C.c_size_t, C.c_int32, C.c_int32, i8p, i32p, i32p, i32p]
    L.ieache_debug_linear_plan.argtypes = [vp, C.c_int, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.ieache_tlwe_extract_device.argtypes = [vp, C.c_size_t, vp, vp, vp, sp]
    L.ieache_debug_cmux_plan.argtypes = [vp, C.c_size_t, C.c_int32, C.POINTER(C.c_int64)]
    L.ieache_tgsw_encrypt.argtypes = [pp, i32p, i32p, C.c_size_t, C.c_double, C.c_uint64, i32p]
    L.ieache_cmux_reference.argtypes = [pp, i32p, C.c_size_t, C.c_size_t, i32p, i32p, i32p, i32p]
    L.ieache_lut_tree_reference.argtypes = [pp, i32p, C.c_size_t, C.c_size_t, C.c_int32, i32p, i32p, C.c_int32, i32p, i32p]
    L.ieache_tlwe_extract_reference.argtypes = [pp, C.c_size_t, i32p, i32p, i32p]
    L.ieache_tlwe_encrypt.argtypes = [pp, i32p, i32p, C.c_size_t, C.c_double, C.c_uint64, i32p]
    L.ieache_tlwe_phase.argtypes = [pp, i32p, i32p, C.c_size_t, i32p]
    L.ieache_lut_factor_poly.argtypes = [pp, C.c_int32, i32p, i32p]
    L.ieache_extract_stride.argtypes = [vp]
    L.ieache_lut_test_poly.argtypes = [pp, C.c_int32, i32p, i32p]
    L.ieache_circuit_gate_count.restype = C.c_int64
    L.ieache_circuit_gate_count.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.ieache_netlist_gate_count.restype = C.c_int64
    L.ieache_netlist_gate_count.argtypes = [vp, C.c_int]
    L.ieache_netlist_create.restype = vp
    L.ieache_netlist_create.argtypes = [C.c_int32, vp, C.c_size_t, i32p, C.c_size_t, C.c_int]
    L.ieache_netlist_destroy.argtypes = [vp]
    L.ieache_program_compile.restype = vp
    L.ieache_program_compile.argtypes = [vp, C.c_size_t, vp, C.c_size_t, u32p, C.c_size_t, i32p, C.c_size_t, C.c_int]
    L.ieache_netlist_export.restype = C.c_int64
    L.ieache_netlist_export.argtypes = [vp, vp, C.c_size_t, i32p, C.c_size_t]
    L.ieache_netlist_info.argtypes = [vp, C.POINTER(CircuitInfo), C.POINTER(C.c_int64)]
    L.ieache_netlist_simulate.argtypes = [vp, u8p, u8p]
    L.ieache_prepare_netlist.argtypes = [vp, vp, C.c_size_t]
    L.ieache_eval_netlist.argtypes = [vp, vp, C.c_size_t, i32p, i32p, sp]
    L.ieache_eval_netlist_device.argtypes = [vp, vp, C.c_size_t, vp, vp, sp]
    jp = C.POINTER(Job)
    L.ieache_prepare_jobs.argtypes = [vp, jp, C.c_size_t]
    L.ieache_eval_jobs.argtypes = [vp, jp, C.c_size_t, sp]
    L.ieache_eval_jobs_device.argtypes = [vp, jp, C.c_size_t, sp]
    L.ieache_group_eval_jobs.argtypes = [vp, jp, C.c_size_t, sp]
    ip = C.POINTER(C.c_int)
    L.ieache_group_create.restype = vp
    L.ieache_group_create.argtypes = [C.c_char_p, ip, C.c_int]
    L.ieache_group_create_raw.restype = vp
    L.ieache_group_create_raw.argtypes = [pp, i32p, i32p, ip, C.c_int]
    L.ieache_group_destroy.restype = None
    L.ieache_group_destroy.argtypes = [vp]
    L.ieache_group_size.argtypes = [vp]
    L.ieache_group_device.argtypes = [vp, C.c_int]
    L.ieache_group_ctx.restype = vp
    L.ieache_group_ctx.argtypes = [vp, C.c_int]
    L.ieache_group_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.ieache_group_prepare_batch.argtypes = [vp, C.c_int, C.c_int, C.c_size_t]
    L.ieache_group_eval_batch.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, i32p, i32p, sp]
    L.ieache_group_prepare_netlist.argtypes = [vp, vp, C.c_size_t]
    L.ieache_group_eval_netlist.argtypes = [vp, vp, C.c_size_t, i32p, i32p, sp]
    L.ieache_group_gates.argtypes = [vp, C.c_int, C.c_size_t, i32p, i32p, i32p, sp]
    L.ieache_group_gates3.argtypes = [vp, C.c_int, C.c_size_t, i32p, i32p, i32p, i32p, sp]
    L.ieache_group_mux.argtypes = [vp, C.c_size_t, i32p, i32p, i32p, i32p, sp]
    L.ieache_group_pbs.argtypes = [vp, C.c_size_t, i32p, i32p, C.c_int32, i32p, i32p, C.c_int, sp]
    L.ieache_group_pbs_multi.argtypes = [vp, C.c_size_t, i32p, i32p, C.c_int32, i32p, i32p, C.c_int32, i32p, i32p, C.c_int, sp]
    L.ieache_debug_blind_rotate.argtypes = [vp, C.c_size_t, i32p, i32p, C.c_int32]
    L.ieache_debug_keyswitch.argtypes = [vp, C.c_size_t, i32p, i32p]
    f64p = C.POINTER(C.c_double)
    L.ieache_debug_twiddles.argtypes = [vp, C.c_int, f64p]
    L.ieache_debug_fft512.argtypes = [vp, C.c_int, C.c_size_t, f64p, f64p]
    L.ieache_debug_spectrum.argtypes = [vp, C.c_int, C.c_size_t, C.c_size_t, f64p]
    L.ieache_debug_forward_path.argtypes = [C.c_int]
    L.ieache_keygen_raw.argtypes = [pp, u32p, C.c_int, i32p, i32p, i32p, i32p]
    L.ieache_keygen_files.argtypes = [C.c_char_p, pp, u32p, C.c_int, u32p, C.c_int]
    L.ieache_encrypt_bits.argtypes = [pp, i32p, u8p, C.c_size_t, C.c_uint64, i32p]
    L.ieache_decrypt_bits.argtypes = [pp, i32p, i32p, C.c_size_t, u8p]
    L.ieache_read_secret_key.argtypes = [C.c_char_p, pp, i32p, i32p]
    L.ieache_read_cloud_key.argtypes = [C.c_char_p, pp, i32p, i32p]
    L.ieache_write_cloud_key.argtypes = [C.c_char_p, pp, i32p, i32p]
    L.ieache_write_secret_key.argtypes = [C.c_char_p, pp, i32p, i32p, i32p, i32p]
    L.ieache_read_samples.argtypes = [C.c_char_p, C.c_int32, C.c_size_t, C.c_size_t, i32p]
    L.ieache_write_samples.argtypes = [C.c_char_p, C.c_int32, C.c_size_t, i32p, C.c_int]
    L.ieache_alice.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, u32p, C.c_uint64]
    L.ieache_verif.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32p, u32p, u32p]
    L.ieache_serve.restype = C.c_int64
    L.ieache_serve.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int64]
    L.ieache_serve_devices.restype = C.c_int64
    L.ieache_serve_devices.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int64]
    L.ieache_debug_mix_plan.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.ieache_shard_slice.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ieache_client_ping.argtypes = [C.c_char_p]
    L.ieache_client_run_dir.argtypes = [C.c_char_p, C.c_char_p]
    L.ieache_client_run_data.argtypes = [C.c_char_p, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ieache_client_shutdown.argtypes = [C.c_char_p]
    _LIB = L
    return L


def check(rc):
    if rc < 0:
        raise IeacheError(rc, lib().ieache_last_error().decode())
    return rc


def _i32(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _opt_i32(a, *shape):
    """an optional int32 array of this shape: None stays None"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(*shape)


def _opt(a):
    """the optional host array of an entry point as its pointer: None is null"""
    return None if a is None else _i32(a)


def _dev(d):
    """the optional device pointer (int) of an entry point: None / 0 is null"""
    return C.c_void_p(d or None)


def _f64(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


# the transform probe's forms (csrc/fft_probe.h): forward 0 .. 4, inverse 5, paired inverses 6 and 7
FFT_FORWARD_FORMS, FFT_INVERSE_FORMS, FFT_PAIRED_FORMS = (0, 1, 2, 3, 4), (5, 6, 7), (6, 7)
TWIDDLE_ENTRIES = 576


def _pbs_flags(keyswitch=True, tlwe=False, accumulator=False):
    return (0 if keyswitch else PBS_NO_KEYSWITCH) | (PBS_TLWE_POLYS if tlwe else 0) | (PBS_ACCUMULATOR if accumulator else 0)


def _pbs_table(params, test_polys, tlwe):
    """the table of a programmable bootstrap as the library takes it: [n_polys][N], or for TLWE samples [n_polys][2][N]"""
    if tlwe:
        return np.ascontiguousarray(test_polys, dtype=np.int32).reshape(-1, 2, params.N)
    return np.ascontiguousarray(test_polys, dtype=np.int32).reshape(-1, params.N)


def _pbs_out(params, count, keyswitch, accumulator):
    if accumulator:
        return np.zeros((count, 2, params.N), dtype=np.int32)
    return np.zeros((count, (params.n if keyswitch else params.N) + 1), dtype=np.int32)


# the row kinds of a linear layer (include/ieache.h section 3n)
ROWS_LWE, ROWS_EXTRACTED, ROWS_TLWE = 0, 1, 2
LINEAR_MAX_DIM = 65536
_ROWS_KINDS = {"lwe": ROWS_LWE, "extracted": ROWS_EXTRACTED, "tlwe": ROWS_TLWE}


def linear_rows_kind(rows):
    """"lwe" / "extracted" / "tlwe", or the number itself (an unknown number goes to the library, which refuses it)"""
    if isinstance(rows, str):
        if rows not in _ROWS_KINDS:
            raise ValueError("lwe_linear: rows must be one of %s" % ", ".join(sorted(_ROWS_KINDS)))
        return _ROWS_KINDS[rows]
    return int(rows)


def linear_row_words(params, rows):
    """words of a host row of that kind: n + 1, N + 1, 2N (None for a kind the library does not know)"""
    return {ROWS_LWE: params.n + 1, ROWS_EXTRACTED: params.N + 1, ROWS_TLWE: 2 * params.N}.get(linear_rows_kind(rows))


def linear_weights(W, bias=None):
    """W as the int8 matrix [n_out][n_in] the library takes and bias as int32 [n_out] or None; ValueError for a weight outside
    -128 .. 127 -- before the library is called -- or a bias of another length"""
    W = np.asarray(W)
    if W.ndim != 2 or not (np.issubdtype(W.dtype, np.integer) or W.dtype == np.bool_):
        raise ValueError("lwe_linear: W must be an integer matrix [n_out][n_in]")
    if W.size and (int(W.min()) < -128 or int(W.max()) > 127):
        raise ValueError("lwe_linear: weights must lie in -128 .. 127 (wider ones: a second call with shifted weights)")
    W = np.ascontiguousarray(W, dtype=np.int8)
    if bias is not None:
        bias = np.ascontiguousarray(np.asarray(bias, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32).view(np.int32).reshape(-1)
        if bias.shape[0] != W.shape[0]:
            raise ValueError("lwe_linear: bias must hold one word per output")
    return W, bias


def _i8(a):
    assert a.dtype == np.int8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int8))


def _stats_ref(stats):
    """the optional Stats argument of an entry point: a reference to it, or a null pointer"""
    return C.byref(stats) if stats is not None else None


def _job_array(jobs, n_words, fold):
    """jobs: (kind, bits, in_lwe) or (CompiledNetlist, in_lwe) each, in_lwe [batch][n_inputs][n+1] on the host
    -> (ieache_job array, the arrays it points into, one output array per job)"""
    arr = (Job * max(len(jobs), 1))()
    ins, outs = [], []
    for i, job in enumerate(jobs):
        if len(job) == 2:
            nl, in_lwe = job
            info = nl.info()
            arr[i].netlist = nl.h
        else:
            kind, bits, in_lwe = job
            info = circuit_info(kind, bits, fold)
            arr[i].kind, arr[i].bits = int(kind), int(bits)
        in_lwe = np.ascontiguousarray(in_lwe, dtype=np.int32)
        batch = in_lwe.shape[0]
        assert in_lwe.shape == (batch, info.n_inputs, n_words), in_lwe.shape
        out = np.zeros((batch, info.n_outputs, n_words), dtype=np.int32)
        arr[i].batch = batch
        arr[i].in_lwe = in_lwe.ctypes.data
        arr[i].out_lwe = out.ctypes.data
        ins.append(in_lwe)
        outs.append(out)
    return arr, ins, outs


def default_params():
    p = Params()
    lib().ieache_default_params(C.byref(p))
    return p


def device_count():
    return lib().ieache_device_count()


def debug_forward_path(xlane):
    """Which form of the forward transforms' lane-high transpose k_blind_rotate_w1b's launches take from here on, in every
    context of the process: 2 (the exchange form, the default) or 1 (the v_cndmask form built beside it).  Same words either
    way: the partner of an A/B and of a test."""
    check(lib().ieache_debug_forward_path(xlane))


def circuit_info(kind, bits, fold=False, level_cap=0):
    info = CircuitInfo()
    check(lib().ieache_circuit_info_get_cap(kind, bits, int(fold), int(level_cap), C.byref(info)))
    return info


def circuit_gate_count(kind, bits, gate_type, fold=False):
    """Gates of one GATE_* type (MAJ3 / XOR3 included) in a built-in circuit."""
    return check(lib().ieache_circuit_gate_count(kind, bits, int(fold), int(gate_type)))


def circuit_level_cap(kind, bits, batch, resident_workgroups=1024, fold=False):
    """Level width for `batch` expressions on a GPU that holds `resident_workgroups` blind rotations at once ("level_quantum");
    0 = the default schedule.  What a given context picks (its device's residency, both kernels): Context.circuit_level_cap."""
    return check(lib().ieache_circuit_level_cap(kind, bits, int(fold), int(batch), int(resident_workgroups)))


def circuit_simulate(kind, bits, in_bits, fold=False, level_cap=0):
    """Plaintext run of the levelised, slot-allocated circuit (host only)."""
    info = circuit_info(kind, bits, fold)
    in_bits = np.ascontiguousarray(in_bits, dtype=np.uint8)
    assert in_bits.shape == (info.n_inputs,)
    out = np.zeros(info.n_outputs, dtype=np.uint8)
    check(lib().ieache_circuit_simulate_cap(kind, bits, int(fold), int(level_cap), in_bits.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


class Netlist:
    """A circuit of your own, recorded gate by gate as a program would call libtfhe's bootsAND / bootsXNOR / bootsMUX ...:

        nl = Netlist(3)
        s = nl.XOR(nl.input(0), nl.input(1))
        out = nl.MUX(nl.input(2), s, NOT(s))
        compiled = nl.compile([out, TRUE])

    Every method returns a reference usable as a later gate's operand or as an output; NOT(ref), TRUE and FALSE are free
    (bootsNOT / bootsCONSTANT).  Nothing is folded: each recorded gate is bootstrapped.  Host only -- no GPU, no context."""

    def __init__(self, n_inputs):
        self.n_inputs = int(n_inputs)
        self._gates = []  # (type, a, b, c)

    def input(self, i):
        if not 0 <= i < self.n_inputs:
            raise IndexError("netlist input %d of %d" % (i, self.n_inputs))
        return int(i) << 1

    def inputs(self, first, count):
        return [self.input(first + i) for i in range(count)]

    def gate(self, gate_type, a, b, c=0):
        """Records one gate and returns the reference of its output; c is the third operand of MUX (a ? b : c), MAJ3 and XOR3."""
        self._gates.append((int(gate_type), int(a), int(b), int(c)))
        return (self.n_inputs + len(self._gates) - 1) << 1

    def AND(self, a, b): return self.gate(GATE_AND, a, b)
    def OR(self, a, b): return self.gate(GATE_OR, a, b)
    def XOR(self, a, b): return self.gate(GATE_XOR, a, b)
    def NAND(self, a, b): return self.gate(GATE_NAND, a, b)
    def NOR(self, a, b): return self.gate(GATE_NOR, a, b)
    def XNOR(self, a, b): return self.gate(GATE_XNOR, a, b)
    def ANDNY(self, a, b): return self.gate(GATE_ANDNY, a, b)
    def ANDYN(self, a, b): return self.gate(GATE_ANDYN, a, b)
    def ORNY(self, a, b): return self.gate(GATE_ORNY, a, b)
    def ORYN(self, a, b): return self.gate(GATE_ORYN, a, b)
    def MUX(self, a, b, c): return self.gate(GATE_MUX, a, b, c)
    # one bootstrap each; three different wires (constants may repeat) -- compile() refuses a repeated wire
    def MAJ3(self, a, b, c): return self.gate(GATE_MAJ3, a, b, c)
    def XOR3(self, a, b, c): return self.gate(GATE_XOR3, a, b, c)

    def __len__(self):
        return len(self._gates)

    def compile(self, outputs, balanced=False):
        """-> CompiledNetlist returning `outputs` (references) per expression.  balanced: the slack-balanced schedule at the
        mean level width instead of ASAP levels.  Raises IeacheError naming the offending gate when the list is not valid."""
        gates = np.ascontiguousarray(np.array(self._gates, dtype=np.int32).reshape(-1, 4))
        outs = np.ascontiguousarray(np.array(list(outputs), dtype=np.int32).reshape(-1))
        h = lib().ieache_netlist_create(self.n_inputs, gates.ctypes.data_as(C.c_void_p), gates.shape[0], _i32(outs), outs.size,
                                        1 if balanced else 0)
        if not h:
            raise IeacheError(-22, lib().ieache_last_error().decode())
        return CompiledNetlist(h, self.n_inputs, list(self._gates), [int(o) for o in outs])


class CompiledNetlist:
    """ieache_netlist: validated, levelised, slot-allocated; what Context.eval_netlist takes.  May be shared by contexts."""

    def __init__(self, handle, n_inputs=0, gates=(), outputs=()):
        self.h = handle
        # the gate list it was compiled from, (type, a, b, c) per gate, and its output references: for walking it elsewhere
        self.n_inputs, self.gates, self.outputs = n_inputs, gates, outputs
        self._info = CircuitInfo()
        self._by_type = (C.c_int64 * GATE_TYPES)()
        check(lib().ieache_netlist_info(self.h, C.byref(self._info), self._by_type))

    def close(self):
        if getattr(self, "h", None):
            lib().ieache_netlist_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        """CircuitInfo; bootstraps and widths count blind rotations (a MUX gate is two)."""
        return self._info

    def gates_by_type(self):
        """Gates recorded, indexed by GATE_* (a MUX counts 1).  MAJ3 / XOR3 lie outside this list: gate_count()."""
        return [int(v) for v in self._by_type]

    def gate_count(self, gate_type):
        """Gates recorded with one GATE_* type, MAJ3 / XOR3 included."""
        return check(lib().ieache_netlist_gate_count(self.h, int(gate_type)))

    def simulate(self, in_bits):
        """Plaintext run (host only): in_bits [n_inputs] -> [n_outputs], each 0/1."""
        in_bits = np.ascontiguousarray(in_bits, dtype=np.uint8)
        assert in_bits.shape == (self._info.n_inputs,), in_bits.shape
        out = np.zeros(self._info.n_outputs, dtype=np.uint8)
        check(lib().ieache_netlist_simulate(self.h, in_bits.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out


class TgswSet:
    """ieache_tgsw: a prepared set of n TGSW samples (Context.tgsw_prepare).  It owns its device memory: close() may come
    before or after the close of the context that prepared it, and only that context accepts it.  l, Bgbit: the set's gadget --
    the context's, or the one given to Context.tgsw_prepare."""

    def __init__(self, handle, n):
        if not handle:
            raise IeacheError(-22, lib().ieache_last_error().decode())
        self.h, self.n = handle, n
        l, Bgbit = C.c_int32(), C.c_int32()
        check(lib().ieache_tgsw_gadget(self.h, C.byref(l), C.byref(Bgbit)))
        self.l, self.Bgbit = l.value, Bgbit.value

    def close(self):
        if getattr(self, "h", None):
            lib().ieache_tgsw_free(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


AUTOMATON_MAX_STATES, AUTOMATON_MAX_STEPS = 64, 4096


def automaton_tables(next0, next1):
    """the transition tables of an automaton as two int32 arrays [steps][states] (one row [states]: one step)"""
    next0, next1 = np.ascontiguousarray(next0, dtype=np.int32), np.ascontiguousarray(next1, dtype=np.int32)
    if next0.ndim == 1:
        next0, next1 = next0.reshape(1, -1), next1.reshape(1, -1)
    if next0.ndim != 2 or next0.shape != next1.shape:
        raise ValueError("automaton: next0 and next1 must both be [steps][states]")
    return next0, next1


class Automaton:
    """ieache_automaton: a compiled deterministic automaton (Context.automaton; include/ieache.h section 3k) -- the public
    transition tables and the live masks on the device.  Like a TgswSet it owns its device memory: close() may come before or
    after the close of the context that compiled it, and only that context accepts it.  states, steps, n_out; cmuxes: the live
    CMuxes per item."""

    def __init__(self, handle):
        if not handle:
            raise IeacheError(-22, lib().ieache_last_error().decode())
        self.h = handle
        st, sp, no, cm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().ieache_automaton_info(self.h, C.byref(st), C.byref(sp), C.byref(no), C.byref(cm)))
        self.states, self.steps, self.n_out, self.cmuxes = st.value, sp.value, no.value, cm.value

    def close(self):
        if getattr(self, "h", None):
            lib().ieache_automaton_free(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context:
    """Cloud key resident on one GPU (ieache_ctx)."""

    def __init__(self, handle):
        if not handle:
            raise IeacheError(-19, lib().ieache_last_error().decode())
        self.h = handle
        self.params = Params()
        check(lib().ieache_ctx_params(self.h, C.byref(self.params)))

    @classmethod
    def from_file(cls, cloud_key_path, device=0):
        return cls(lib().ieache_ctx_create(os.fsencode(cloud_key_path), device))

    @classmethod
    def from_arrays(cls, params, bk, ksk, device=0):
        bk = np.ascontiguousarray(bk, dtype=np.int32)
        ksk = np.ascontiguousarray(ksk, dtype=np.int32)
        assert bk.size == params.bk_count and ksk.size == params.ksk_count
        return cls(lib().ieache_ctx_create_raw(C.byref(params), _i32(bk), _i32(ksk), device))

    @classmethod
    def from_device_pointers(cls, params, d_bk, d_ksk, device=0):
        """d_bk / d_ksk: integer device addresses (e.g. torch tensor .data_ptr())."""
        return cls(lib().ieache_ctx_create_device(C.byref(params), C.c_void_p(d_bk), C.c_void_p(d_ksk), device))

    def close(self):
        if getattr(self, "h", None):
            lib().ieache_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def lwe_stride(self):
        return lib().ieache_lwe_stride(self.h)

    @property
    def stream(self):
        return lib().ieache_ctx_stream(self.h)

    @property
    def kernel_variant(self):
        return lib().ieache_ctx_kernel_variant(self.h).decode()

    def kernel_for_launch(self, gates):
        """Name of the blind-rotation kernel a launch of `gates` gate instances takes."""
        return lib().ieache_ctx_kernel_for_launch(self.h, int(gates)).decode()

    def fft_guard(self):
        """(largest distance to an integer the one-limb blind rotation rounded away -- 0.5 would be a wrong bit --,
        calls repeated on the two-limb kernel because a launch exceeded 1/16)."""
        m, r = C.c_double(0), C.c_int64(0)
        check(lib().ieache_ctx_fft_guard(self.h, C.byref(m), C.byref(r)))
        return m.value, r.value

    def circuit_level_cap(self, kind, bits, batch):
        """Level width this context's eval_batch* uses for `batch` expressions; 0 = the default schedule."""
        return check(lib().ieache_ctx_circuit_level_cap(self.h, kind, bits, int(batch)))

    def fft_audit(self):
        """The sampled bit-for-bit audit of the one-limb kernel against the two-limb one (option "fft_audit" = K):
        {"audits": launches audited, "gates_compared": gate instances re-run and compared, "mismatches": rows that differed}."""
        a, g, m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().ieache_ctx_fft_audit(self.h, C.byref(a), C.byref(g), C.byref(m)))
        return {"audits": a.value, "gates_compared": g.value, "mismatches": m.value}

    def set_chunk(self, items):
        check(lib().ieache_ctx_set_chunk(self.h, items))

    def set_option(self, name, value):
        """Tuning knobs: chunk, force_generic, ks_batch_min, br_slice, ..., fold_constants."""
        check(lib().ieache_ctx_set_option(self.h, name.encode(), int(value)))
        if name == "fold_constants":
            self._fold = bool(value)

    def set_option_ok(self, name, value):
        """set_option without raising: False when the name is unknown or the value out of range (nothing is changed then)."""
        return lib().ieache_ctx_set_option(self.h, name.encode(), int(value)) == 0

    def get_option(self, name):
        """Current value of an option, or of a read-only figure ("cus", "resident_gates", "overlapped_levels")."""
        v = C.c_int64(0)
        check(lib().ieache_ctx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def wait_stream(self, hip_stream=None):
        """Order the context's stream after the work queued on `hip_stream` (int handle; None = default stream)."""
        check(lib().ieache_ctx_wait_stream(self.h, C.c_void_p(hip_stream)))

    def force_generic(self, on=True):
        check(lib().ieache_ctx_force_generic(self.h, int(on)))

    def cloud_run(self, workdir):
        return check(lib().ieache_ctx_cloud_run(self.h, os.fsencode(workdir)))

    def eval_batch(self, kind, bits, in_lwe, stats=None):
        """in_lwe [batch][n_inputs][n+1] int32 on the host -> [batch][n_outputs][n+1]."""
        info = circuit_info(kind, bits, getattr(self, "_fold", False))
        in_lwe = np.ascontiguousarray(in_lwe, dtype=np.int32)
        batch = in_lwe.shape[0]
        assert in_lwe.shape == (batch, info.n_inputs, self.params.n + 1), in_lwe.shape
        out = np.zeros((batch, info.n_outputs, self.params.n + 1), dtype=np.int32)
        check(lib().ieache_eval_batch(self.h, kind, bits, batch, _i32(in_lwe), _i32(out), _stats_ref(stats)))
        return out

    def prepare(self, kind, bits, batch):
        """Allocates what eval_batch* of this circuit and batch needs (circuit tables, wire store, scratch), so that a timed
        first evaluation measures the steady state."""
        check(lib().ieache_prepare_batch(self.h, kind, bits, batch))

    def eval_batch_device(self, kind, bits, batch, d_in, d_out, stats=None):
        """Device pointers (ints); rows of lwe_stride int32."""
        check(lib().ieache_eval_batch_device(self.h, kind, bits, batch, C.c_void_p(d_in), C.c_void_p(d_out), _stats_ref(stats)))

    def eval_netlist(self, nl, in_lwe, stats=None):
        """A CompiledNetlist over a batch: in_lwe [batch][n_inputs][n+1] int32 on the host -> [batch][n_outputs][n+1]."""
        info = nl.info()
        in_lwe = np.ascontiguousarray(in_lwe, dtype=np.int32)
        batch = in_lwe.shape[0]
        assert in_lwe.shape == (batch, info.n_inputs, self.params.n + 1), in_lwe.shape
        out = np.zeros((batch, info.n_outputs, self.params.n + 1), dtype=np.int32)
        check(lib().ieache_eval_netlist(self.h, nl.h, batch, _i32(in_lwe), _i32(out), _stats_ref(stats)))
        return out

    def eval_jobs(self, jobs, stats=None):
        """Several circuits' batches together, level by level, so that their narrow levels share every launch (include/ieache.h,
        section 3c).  jobs: (kind, bits, in_lwe) or (CompiledNetlist, in_lwe) each, in_lwe as eval_batch / eval_netlist take it
        -> one output array per job, each word for word what the job gives alone."""
        jobs = list(jobs)
        arr, _ins, outs = _job_array(jobs, self.params.n + 1, getattr(self, "_fold", False))
        check(lib().ieache_eval_jobs(self.h, arr, len(jobs), _stats_ref(stats)))
        return outs

    def eval_jobs_device(self, jobs, stats=None):
        """eval_jobs on device rows of lwe_stride int32: (kind, bits, batch, d_in, d_out) or (CompiledNetlist, batch, d_in, d_out)
        each, pointers as ints."""
        jobs = list(jobs)
        arr = (Job * max(len(jobs), 1))()
        for i, job in enumerate(jobs):
            if len(job) == 4:
                arr[i].netlist = job[0].h
            else:
                arr[i].kind, arr[i].bits = int(job[0]), int(job[1])
            arr[i].batch, arr[i].in_lwe, arr[i].out_lwe = int(job[-3]), job[-2], job[-1]
        check(lib().ieache_eval_jobs_device(self.h, arr, len(jobs), _stats_ref(stats)))

    def prepare_jobs(self, jobs):
        """Allocates what eval_jobs of these jobs needs: (kind, bits, batch) or (CompiledNetlist, batch) each."""
        arr = (Job * max(len(jobs), 1))()
        for i, job in enumerate(jobs):
            if len(job) == 2:
                arr[i].netlist, arr[i].batch = job[0].h, int(job[1])
            else:
                arr[i].kind, arr[i].bits, arr[i].batch = int(job[0]), int(job[1]), int(job[2])
        check(lib().ieache_prepare_jobs(self.h, arr, len(jobs)))

    def prepare_netlist(self, nl, batch):
        """Allocates what eval_netlist* of this netlist and batch needs, so that the evaluation itself allocates nothing."""
        check(lib().ieache_prepare_netlist(self.h, nl.h, batch))

    def eval_netlist_device(self, nl, batch, d_in, d_out, stats=None):
        """Device pointers (ints); rows of lwe_stride int32."""
        check(lib().ieache_eval_netlist_device(self.h, nl.h, batch, C.c_void_p(d_in), C.c_void_p(d_out), _stats_ref(stats)))

    def gates(self, gate_type, a, b, stats=None):
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.ascontiguousarray(b, dtype=np.int32)
        assert a.shape == b.shape and a.shape[-1] == self.params.n + 1
        out = np.zeros_like(a)
        count = a.size // (self.params.n + 1)
        check(lib().ieache_gates(self.h, gate_type, count, _i32(a), _i32(b), _i32(out), _stats_ref(stats)))
        return out

    def gates_device(self, gate_type, count, d_a, d_b, d_out, stats=None):
        check(lib().ieache_gates_device(self.h, gate_type, count, C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_out), _stats_ref(stats)))

    def gates3(self, gate_type, a, b, c, stats=None):
        """GATE_MAJ3 / GATE_XOR3 on host rows: out[i] = gate(a[i], b[i], c[i]), one bootstrap per gate."""
        a, b, c = (np.ascontiguousarray(v, dtype=np.int32) for v in (a, b, c))
        assert a.shape == b.shape == c.shape and a.shape[-1] == self.params.n + 1
        out = np.zeros_like(a)
        check(lib().ieache_gates3(self.h, gate_type, a.size // (self.params.n + 1), _i32(a), _i32(b), _i32(c), _i32(out), _stats_ref(stats)))
        return out

    def gates3_device(self, gate_type, count, d_a, d_b, d_c, d_out, stats=None):
        check(lib().ieache_gates3_device(self.h, gate_type, count, C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c),
                                         C.c_void_p(d_out), _stats_ref(stats)))

    @property
    def extract_stride(self):
        """int32 per device row of extracted samples (pbs_device with keyswitch=False): N + 1 rounded up to a multiple of 4."""
        return lib().ieache_extract_stride(self.h)

    def pbs(self, x, test_polys, poly_of=None, keyswitch=True, stats=None, tlwe=False, accumulator=False):
        """Programmable bootstrap on host rows: x [count][n+1] is bootstrapped row by row as it stands from the test polynomial
        test_polys[poly_of[i]] (test_polys [n_polys][N] or one polynomial [N]; poly_of None: row 0 for every row).  With the
        row's mod-switched phase phi in [0, 2N) the result encrypts v[phi] for phi < N and -v[phi - N] otherwise
        (include/ieache.h; tools.lut_test_poly builds v from a table) -> [count][n+1], or with keyswitch=False the
        extracted samples [count][N+1] under the ring key.
        tlwe=True: test_polys is [n_polys][2][N] (or one [2][N]), TLWE samples under the ring key (tools.tlwe_encrypt of a
        table): the rotation starts from X^(2N-barb) (A, B).  accumulator=True: the whole rotated accumulators
        [count][2][N] are the result, no extraction and no key switch (tools.tlwe_phase reads them)."""
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.params.n + 1)
        tv = _pbs_table(self.params, test_polys, tlwe)
        of = None if poly_of is None else np.ascontiguousarray(poly_of, dtype=np.int32).reshape(-1)
        assert of is None or of.shape[0] == x.shape[0]
        out = _pbs_out(self.params, x.shape[0], keyswitch, accumulator)
        check(lib().ieache_pbs(self.h, x.shape[0], _i32(x), _i32(tv), tv.shape[0], None if of is None else _i32(of), _i32(out),
                               _pbs_flags(keyswitch, tlwe, accumulator), _stats_ref(stats)))
        return out

    def pbs_device(self, count, d_x, d_test_polys, n_polys, d_poly_of, d_out, keyswitch=True, stats=None, tlwe=False, accumulator=False):
        """Device pointers (ints; d_poly_of may be None / 0): x rows of lwe_stride, test polynomials [n_polys][N] packed
        (tlwe=True: [n_polys][2][N]), out rows of lwe_stride or, with keyswitch=False, of extract_stride (accumulator=True:
        packed rows of 2N)."""
        check(lib().ieache_pbs_device(self.h, count, C.c_void_p(d_x), C.c_void_p(d_test_polys), int(n_polys),
                                      C.c_void_p(d_poly_of or None), C.c_void_p(d_out), _pbs_flags(keyswitch, tlwe, accumulator), _stats_ref(stats)))

    def keyswitch(self, u, stats=None):
        """lweKeySwitch on host rows: extracted samples u [count][N+1] under the ring key (what pbs(..., keyswitch=False) returns,
        or sums of such rows) -> [count][n+1] under the LWE key."""
        u = np.ascontiguousarray(u, dtype=np.int32).reshape(-1, self.params.N + 1)
        out = np.zeros((u.shape[0], self.params.n + 1), dtype=np.int32)
        check(lib().ieache_keyswitch(self.h, u.shape[0], _i32(u), _i32(out), _stats_ref(stats)))
        return out

    def keyswitch_device(self, count, d_u, d_out, stats=None):
        """Device pointers (ints): d_u rows of extract_stride, d_out rows of lwe_stride."""
        check(lib().ieache_keyswitch_device(self.h, count, C.c_void_p(d_u), C.c_void_p(d_out), _stats_ref(stats)))

    def _gadget(self, l, Bgbit):
        if (l is None) != (Bgbit is None):
            raise ValueError("tgsw_prepare: give both l and Bgbit, or neither")
        return None if l is None else (int(l), int(Bgbit))

    def tgsw_prepare(self, samples, l=None, Bgbit=None):
        """A prepared set of TGSW samples [n][2l][2][N] (or one [2l][2][N]; tools.tgsw_encrypt, or rows bk[i] of a key) for
        cmux() and lut_tree(): a TgswSet, to be closed (or used as a context manager) before or after this context.
        l, Bgbit: the gadget the samples were made with (tools.tgsw_encrypt on tools.with_gadget(params, l, Bgbit)), any
        admissible one whatever the key's (include/ieache.h section 3i); None: the context's."""
        gadget = self._gadget(l, Bgbit)
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        per = (self.params.k + 1) * (self.params.l if gadget is None else max(gadget[0], 0)) * 2 * self.params.N
        if per and samples.size % per:
            raise ValueError("tgsw_prepare: %d words are no whole number of samples [2l][2][N] with 2l = %d rows" % (samples.size, per // (2 * self.params.N)))
        if gadget is None:
            samples = samples.reshape(-1, per // (2 * self.params.N), 2, self.params.N)
            return TgswSet(lib().ieache_tgsw_prepare(self.h, _i32(samples), samples.shape[0]), samples.shape[0])
        n = samples.size // per if per else 0
        return TgswSet(lib().ieache_tgsw_prepare_gadget(self.h, _i32(samples), n, gadget[0], gadget[1]), n)

    def tgsw_prepare_device(self, d_samples, n, l=None, Bgbit=None):
        """Device pointer (int): samples [n][2l][2][N] packed; l, Bgbit as for tgsw_prepare."""
        gadget = self._gadget(l, Bgbit)
        if gadget is None:
            return TgswSet(lib().ieache_tgsw_prepare_device(self.h, C.c_void_p(d_samples), int(n)), int(n))
        return TgswSet(lib().ieache_tgsw_prepare_gadget_device(self.h, C.c_void_p(d_samples), int(n), gadget[0], gadget[1]), int(n))

    def cmux(self, tgsw, d1, d0=None, sel_of=None, stats=None):
        """CMux on host rows: out[i] = d0[i] + C [.] (d1[i] - d0[i]) with C = sample sel_of[i] of the set (None: i mod n), rows
        [count][2][N]; d0 None: zeros, the external product alone (include/ieache.h section 3f)."""
        d1 = np.ascontiguousarray(d1, dtype=np.int32).reshape(-1, 2, self.params.N)
        count = d1.shape[0]
        d0 = _opt_i32(d0, -1, 2, self.params.N)
        of = _opt_i32(sel_of, -1)
        assert (d0 is None or d0.shape[0] == count) and (of is None or of.shape[0] == count)
        out = np.zeros((count, 2, self.params.N), dtype=np.int32)
        check(lib().ieache_cmux(self.h, tgsw.h, count, _opt(of), _i32(d1), _opt(d0), _i32(out), _stats_ref(stats)))
        return out

    def cmux_device(self, tgsw, count, d_sel_of, d_d1, d_d0, d_out, stats=None):
        """Device pointers (ints; d_sel_of and d_d0 may be None / 0): rows [count][2][N] packed, indices [count] int32."""
        check(lib().ieache_cmux_device(self.h, tgsw.h, count, _dev(d_sel_of), C.c_void_p(d_d1), _dev(d_d0), C.c_void_p(d_out), _stats_ref(stats)))

    def lut_tree(self, tgsw, tables, depth, sel_of=None, table_of=None, count=None, stats=None):
        """CMux-tree lookup on host rows: item i folds tables[table_of[i]] (tables [n_tables][2^depth][2][N] or one table;
        table_of None: table 0) by the selectors sel_of[i] ([count][depth], bit k of the index first; None: samples
        i depth + k mod n) -> [count][2][N], an encryption of the table's row at the encrypted index.  count: the number of
        items where neither index array gives it (default 1)."""
        depth = int(depth)
        tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
        of = _opt_i32(sel_of, -1, max(depth, 1))
        tof = _opt_i32(table_of, -1)
        if count is None:
            count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth > 0 else 1)
        assert (tof is None or tof.shape[0] == count) and (of is None or depth < 1 or of.shape[0] == count)
        out = np.zeros((count, 2, self.params.N), dtype=np.int32)
        check(lib().ieache_lut_tree(self.h, tgsw.h, count, depth, _opt(of), _i32(tables), tables.shape[0], _opt(tof), _i32(out), _stats_ref(stats)))
        return out

    def lut_tree_device(self, tgsw, count, depth, d_sel_of, d_tables, n_tables, d_table_of, d_out, stats=None):
        """Device pointers (ints; the index arrays may be None / 0): tables [n_tables][2^depth][2][N] packed, out [count][2][N]."""
        check(lib().ieache_lut_tree_device(self.h, tgsw.h, count, int(depth), _dev(d_sel_of), C.c_void_p(d_tables), int(n_tables),
                                           _dev(d_table_of), C.c_void_p(d_out), _stats_ref(stats)))

    def lut_scatter(self, tgsw, values, depth, sel_of=None, mem=None, count=None, stats=None):
        """The write at an encrypted index on host rows (include/ieache.h section 3g), lut_tree's partner: item i
        demultiplexes values[i] ([count][2][N], or one row) by the selectors sel_of[i] ([count][depth], bit k of the index
        first as for lut_tree; None: samples i depth + k mod n) and returns mem[i] + leaves ([count][2^depth][2][N]): values[i]
        added at the encrypted index, encryptions of zero elsewhere.  mem None: zeros, the leaves themselves.  count: checked
        against the rows of values where given."""
        depth = int(depth)
        values = np.ascontiguousarray(values, dtype=np.int32).reshape(-1, 2, self.params.N)
        n = values.shape[0] if count is None else int(count)
        of = _opt_i32(sel_of, -1, max(depth, 1))
        mem = _opt_i32(mem, -1, 1 << max(depth, 0), 2, self.params.N)
        assert values.shape[0] == n and (of is None or depth < 1 or of.shape[0] == n) and (mem is None or mem.shape[0] == n)
        out = np.zeros((n, 1 << max(depth, 0), 2, self.params.N), dtype=np.int32)
        check(lib().ieache_lut_scatter(self.h, tgsw.h, n, depth, _opt(of), _i32(values), _opt(mem), _i32(out), _stats_ref(stats)))
        return out

    def lut_scatter_device(self, tgsw, count, depth, d_sel_of, d_values, d_mem, d_out, stats=None):
        """Device pointers (ints; d_sel_of and d_mem may be None / 0): values [count][2][N], mem and out [count][2^depth][2][N]
        packed; d_out == d_mem writes in place."""
        check(lib().ieache_lut_scatter_device(self.h, tgsw.h, count, int(depth), _dev(d_sel_of), C.c_void_p(d_values),
                                              _dev(d_mem), C.c_void_p(d_out), _stats_ref(stats)))

    def lut_write(self, tgsw, mem, depth, new, sel_of=None):
        """The replace write mem[i][addr_i] := new[i] on host arrays, addr_i the index item i's selectors encrypt: a read
        (lut_tree with table_of = arange(count)), a wrapping subtraction and lut_scatter of the difference.  mem
        [count][2^depth][2][N], new [count][2][N] -> the new memory.  The addressed slot ends at new plus the noise of a tree and a
        scatter; every other slot gains a scatter's."""
        depth = int(depth)
        mem = np.ascontiguousarray(mem, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
        new = np.ascontiguousarray(new, dtype=np.int32).reshape(-1, 2, self.params.N)
        count = mem.shape[0]
        assert new.shape[0] == count
        old = self.lut_tree(tgsw, mem, depth, sel_of=sel_of, table_of=np.arange(count, dtype=np.int32), count=count)
        delta = ((new.astype(np.int64) - old.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        return self.lut_scatter(tgsw, delta, depth, sel_of=sel_of, mem=mem, count=count)

    def lut_write_device(self, tgsw, count, depth, d_sel_of, d_new, d_mem, d_out, stats=None):
        """The replace write on the device (include/ieache.h section 3i), word for word lut_write's composition with no host round
        trip.  Device pointers (ints; d_sel_of may be None / 0): new [count][2][N], mem and out [count][2^depth][2][N] packed;
        d_out == d_mem writes in place."""
        check(lib().ieache_lut_write_device(self.h, tgsw.h, count, int(depth), _dev(d_sel_of), C.c_void_p(d_new), C.c_void_p(d_mem),
                                            C.c_void_p(d_out), _stats_ref(stats)))

    def tlwe_rotate(self, tgsw, rows, steps, sel_of=None, amounts=None, stats=None):
        """Rotation by an encrypted amount on host rows (include/ieache.h section 3h): row i ([count][2][N], or one row) goes
        through acc <- acc + C_t [.] (X^(a_t) acc - acc) for t = 0 .. steps-1, C_t = sample sel_of[i][t] of the set
        ([count][steps]; None: samples i steps + t mod n), a_t = amounts[t] in [0, 2N) shared by all rows (None: 2N - 2^t, which
        brings coefficient sum b_t 2^t to position 0; tools.rotate_amounts gives both directions)."""
        steps = int(steps)
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2, self.params.N)
        count = rows.shape[0]
        of = _opt_i32(sel_of, -1, max(steps, 1))
        am = _opt_i32(amounts, -1)
        assert (of is None or steps < 1 or of.shape[0] == count) and (am is None or am.shape[0] == max(steps, 0))
        out = np.zeros((count, 2, self.params.N), dtype=np.int32)
        check(lib().ieache_tlwe_rotate(self.h, tgsw.h, count, steps, _opt(of), _opt(am), _i32(rows), _i32(out), _stats_ref(stats)))
        return out

    def tlwe_rotate_device(self, tgsw, count, steps, d_sel_of, d_amounts, d_in, d_out, stats=None):
        """Device pointers (ints; d_sel_of and d_amounts may be None / 0): rows [count][2][N] packed, selectors [count][steps] and
        amounts [steps] int32; d_out == d_in rotates in place."""
        check(lib().ieache_tlwe_rotate_device(self.h, tgsw.h, count, int(steps), _dev(d_sel_of), _dev(d_amounts),
                                              C.c_void_p(d_in), C.c_void_p(d_out), _stats_ref(stats)))

    def lut_read(self, tgsw, tables, depth, steps, sel_of=None, amounts=None, table_of=None, coef=0, keyswitch=True, count=None, stats=None):
        """The coefficient-level lookup on host rows (section 3h): item i looks up tables[table_of[i]] ([n_tables][2^depth][2][N])
        by its depth + steps address bits sel_of[i] ([count][steps + depth]: the `steps` LOW bits first, least significant first,
        then the `depth` HIGH ones; None: samples i (steps + depth) + t mod n) -- a CMux tree by the high bits, the rotation of the
        selected sample by the low bits, coefficient `coef` extracted and key-switched -> LWE rows [count][n+1] (keyswitch=False:
        the extracted rows [count][N+1])."""
        depth, steps = int(depth), int(steps)
        tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
        of = _opt_i32(sel_of, -1, max(depth + steps, 1))
        am = _opt_i32(amounts, -1)
        tof = _opt_i32(table_of, -1)
        if count is None:
            count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth + steps > 0 else 1)
        assert (tof is None or tof.shape[0] == count) and (of is None or depth + steps < 1 or of.shape[0] == count)
        assert am is None or am.shape[0] == max(steps, 0)
        out = np.zeros((count, (self.params.n if keyswitch else self.params.N) + 1), dtype=np.int32)
        check(lib().ieache_lut_read(self.h, tgsw.h, count, depth, steps, _opt(of), _opt(am), _i32(tables), tables.shape[0], _opt(tof), int(coef),
                                    0 if keyswitch else LUT_READ_NO_KEYSWITCH, _i32(out), _stats_ref(stats)))
        return out

    def lut_read_device(self, tgsw, count, depth, steps, d_sel_of, d_amounts, d_tables, n_tables, d_table_of, d_out, coef=0, keyswitch=True, stats=None):
        """Device pointers (ints; the index arrays and d_amounts may be None / 0): tables [n_tables][2^depth][2][N] packed, out rows
        of lwe_stride words (keyswitch=False: of extract_stride words)."""
        check(lib().ieache_lut_read_device(self.h, tgsw.h, count, int(depth), int(steps), _dev(d_sel_of), _dev(d_amounts),
                                           C.c_void_p(d_tables), int(n_tables), _dev(d_table_of), int(coef),
                                           0 if keyswitch else LUT_READ_NO_KEYSWITCH, C.c_void_p(d_out), _stats_ref(stats)))

    def lut_add(self, tgsw, values, depth, steps=0, sel_of=None, amounts=None, mems=None, n_mems=1, mem_of=None, stats=None):
        """Many values into shared memories in one call (include/ieache.h section 3j): mem[m_i][hi_i].coef[lo_i] += values[i].
        values [count][2][N] (or one row); sel_of [count][steps + depth], the `steps` LOW address bits first, then the `depth` HIGH
        ones (None: samples i (steps + depth) + t mod n); amounts [steps] (None: +2^t mod 2N, which moves coefficient 0 to the
        encrypted position); mems [n_mems][2^depth][2][N] (None: zeros; given, it fixes n_mems); mem_of [count] (None: memory 0)
        -> the new memories [n_mems][2^depth][2][N].  Word for word tlwe_rotate, lut_scatter(mem=None) and the sum of the leaves
        per memory, which the last demux step forms on the device."""
        depth, steps = int(depth), int(steps)
        values = np.ascontiguousarray(values, dtype=np.int32).reshape(-1, 2, self.params.N)
        count = values.shape[0]
        of = _opt_i32(sel_of, -1, max(depth + steps, 1))
        am = _opt_i32(amounts, -1)
        mof = _opt_i32(mem_of, -1)
        if mems is not None:
            mems = np.ascontiguousarray(mems, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
            n_mems = mems.shape[0]
        n_mems = int(n_mems)
        assert (of is None or depth + steps < 1 or of.shape[0] == count) and (am is None or am.shape[0] == max(steps, 0))
        assert mof is None or mof.shape[0] == count
        out = np.zeros((max(n_mems, 0), 1 << max(depth, 0), 2, self.params.N), dtype=np.int32)
        check(lib().ieache_lut_add(self.h, tgsw.h, count, depth, steps, _opt(of), _opt(am), _i32(values), _opt(mems), n_mems, _opt(mof), _i32(out),
                                   _stats_ref(stats)))
        return out

    def lut_add_device(self, tgsw, count, depth, steps, d_sel_of, d_amounts, d_values, d_mems, n_mems, d_mem_of, d_out, stats=None):
        """Device pointers (ints; the index arrays, d_amounts and d_mems may be None / 0): values [count][2][N], mems and out
        [n_mems][2^depth][2][N] packed; d_out == d_mems adds in place."""
        check(lib().ieache_lut_add_device(self.h, tgsw.h, count, int(depth), int(steps), _dev(d_sel_of), _dev(d_amounts), C.c_void_p(d_values),
                                          _dev(d_mems), int(n_mems), _dev(d_mem_of), C.c_void_p(d_out), _stats_ref(stats)))

    def automaton(self, next0, next1, n_out=1):
        """Compile a deterministic automaton (include/ieache.h section 3k): next0, next1 [steps][states] int32, the state after
        reading letter 0 / 1 at step t from state q (they may differ from step to step; ieache_amd.automata has worked examples);
        outputs for the start states 0 .. n_out-1 -> an Automaton, to be closed (or used as a context manager) before or after
        this context."""
        next0, next1 = automaton_tables(next0, next1)
        return Automaton(lib().ieache_automaton_create(self.h, next0.shape[1], next0.shape[0], int(n_out), _i32(next0), _i32(next1)))

    def automaton_run(self, tgsw, a, finals, sel_of=None, final_of=None, count=None, stats=None):
        """Run an automaton on words of TGSW-encrypted letters, host rows: item i starts from V_steps = finals[final_of[i]]
        (finals [n_finals][states][2][N] or one [states][2][N]; final_of None: 0) and folds backward by the selectors sel_of[i]
        ([count][steps], letter t the one read t-th; None: samples i steps + t mod n) -> [count][n_out][2][N]: out[i][q]
        encrypts the final row the run from state q over item i's word ends in.  count: the number of items where neither
        index array gives it (default 1)."""
        N = self.params.N
        finals = np.ascontiguousarray(finals, dtype=np.int32).reshape(-1, a.states, 2, N)
        of = _opt_i32(sel_of, -1, max(a.steps, 1))
        fof = _opt_i32(final_of, -1)
        if count is None:
            count = fof.shape[0] if fof is not None else (of.shape[0] if of is not None and a.steps > 0 else 1)
        assert (fof is None or fof.shape[0] == count) and (of is None or a.steps < 1 or of.shape[0] == count)
        out = np.zeros((count, a.n_out, 2, N), dtype=np.int32)
        check(lib().ieache_automaton_run(self.h, tgsw.h, a.h, count, _opt(of), _i32(finals), finals.shape[0], _opt(fof), _i32(out), _stats_ref(stats)))
        return out

    def automaton_run_device(self, tgsw, a, count, d_sel_of, d_finals, n_finals, d_final_of, d_out, stats=None):
        """Device pointers (ints; the index arrays may be None / 0): finals [n_finals][states][2][N], out [count][n_out][2][N]
        packed; no overlap of out with an input is accepted."""
        check(lib().ieache_automaton_run_device(self.h, tgsw.h, a.h, count, _dev(d_sel_of), C.c_void_p(d_finals), int(n_finals), _dev(d_final_of),
                                                C.c_void_p(d_out), _stats_ref(stats)))

    def automaton_plan(self, a, count):
        """How automaton_run() would cut such a call under the options as they are (csrc/automaton_plan.h): dict(pieces,
        items_per_piece, scratch_rows, steps_per_launch, launches) -- launches per piece."""
        out = (C.c_int64 * 5)()
        check(lib().ieache_debug_automaton_plan(self.h, a.h, count, out))
        return dict(zip(("pieces", "items_per_piece", "scratch_rows", "steps_per_launch", "launches"), (int(v) for v in out)))

    def cmux_plan(self, count, depth=-1):
        """How cmux() (depth < 0) or lut_tree() / lut_scatter() would cut such a call under the options as they are (csrc/cmux_plan.h):
        dict(pieces, items_per_piece, scratch_a_rows, scratch_b_rows)."""
        out = (C.c_int64 * 4)()
        check(lib().ieache_debug_cmux_plan(self.h, count, int(depth), out))
        return dict(zip(("pieces", "items_per_piece", "scratch_a_rows", "scratch_b_rows"), (int(v) for v in out)))

    def tlwe_extract(self, tlwe, coef_of=None, stats=None):
        """Coefficient coef_of[i] (None: 0) of TLWE samples [count][2][N] as extracted rows [count][N+1]: what keyswitch() takes."""
        tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, self.params.N)
        of = _opt_i32(coef_of, -1)
        assert of is None or of.shape[0] == tlwe.shape[0]
        u = np.zeros((tlwe.shape[0], self.params.N + 1), dtype=np.int32)
        check(lib().ieache_tlwe_extract(self.h, tlwe.shape[0], _i32(tlwe), _opt(of), _i32(u), _stats_ref(stats)))
        return u

    def tlwe_extract_device(self, count, d_tlwe, d_coef_of, d_u, stats=None):
        """Device pointers (ints; d_coef_of may be None / 0): samples [count][2][N] packed, d_u rows of extract_stride."""
        check(lib().ieache_tlwe_extract_device(self.h, count, C.c_void_p(d_tlwe), _dev(d_coef_of), C.c_void_p(d_u), _stats_ref(stats)))

    def lwe_linear(self, x, W, bias=None, rows="lwe", stats=None):
        """A linear layer on host rows (include/ieache.h section 3n): x [batch][n_in][words] (or [n_in][words] for one batch
        element), W an integer matrix [n_out][n_in] with values in -128 .. 127, bias [n_out] Torus32 words or None, rows "lwe"
        (n + 1 words, bias on b), "extracted" (N + 1) or "tlwe" (2N, no bias) -> out[b][i] = sum_j W[i][j] x[b][j] (+ bias[i])
        mod 2^32, [batch][n_out][words]."""
        kind = linear_rows_kind(rows)
        W, bias = linear_weights(W, bias)
        x = np.ascontiguousarray(x, dtype=np.int32)
        words = linear_row_words(self.params, kind)
        if words is not None:
            if x.ndim < 2 or x.shape[-1] != words or x.shape[-2] != W.shape[1]:
                raise ValueError("lwe_linear: x must be [batch][n_in = %d][words = %d]" % (W.shape[1], words))
            x = x.reshape(-1, W.shape[1], words)
        out = np.zeros((x.shape[0], W.shape[0], x.shape[-1]), dtype=np.int32)
        check(lib().ieache_lwe_linear(self.h, kind, x.shape[0], W.shape[0], W.shape[1], _i8(W), _opt(bias), _i32(x), _i32(out), _stats_ref(stats)))
        return out

    def lwe_linear_device(self, rows, batch, n_out, n_in, d_w, d_bias, d_x, d_out, stats=None):
        """Device pointers (ints): d_w int8 [n_out][n_in], d_bias int32 [n_out] or None, d_x [batch][n_in] and d_out
        [batch][n_out] rows of the kind's stride (lwe_stride, extract_stride, 2N).  Runs on the context's stream."""
        check(lib().ieache_lwe_linear_device(self.h, linear_rows_kind(rows), batch, int(n_out), int(n_in), C.c_void_p(d_w), _dev(d_bias),
                                             C.c_void_p(d_x), C.c_void_p(d_out), _stats_ref(stats)))

    def linear_plan(self, rows, batch, n_out, n_in):
        """What such a call takes under "linear_kernel" as it is (csrc/linear_plan.h): dict(kernel -- 1 simple, 2 MFMA --,
        col_blocks, wave_tiles, k_steps)."""
        out = (C.c_int64 * 4)()
        check(lib().ieache_debug_linear_plan(self.h, linear_rows_kind(rows), int(batch), int(n_out), int(n_in), out))
        return dict(zip(("kernel", "col_blocks", "wave_tiles", "k_steps"), (int(v) for v in out)))

    def set_packing_key(self, pk, t=8, basebit=2):
        """The packing key [n][t][2][N] (tools.packing_keygen) for pack(): replaces an earlier one; pk=None drops it."""
        if pk is None:
            check(lib().ieache_ctx_set_packing_key(self.h, 0, 0, None))
            return
        pk = np.ascontiguousarray(pk, dtype=np.int32)
        if int(t) >= 1 and pk.size != self.params.n * int(t) * 2 * self.params.N:  # (t < 1: the library refuses it)
            raise ValueError("packing key: expected [n][t][2][N] = %d words, got %d" % (self.params.n * t * 2 * self.params.N, pk.size))
        check(lib().ieache_ctx_set_packing_key(self.h, int(t), int(basebit), _i32(pk)))

    def pack(self, rows, m=None, spread=1, shift=0, stats=None):
        """Packing key switch on host rows: rows [groups][m][n+1] (or [m][n+1] for one group; or any [..][n+1] with m given)
        -> TLWE samples [groups][2][N] whose phase holds row p's phase on coefficients p spread + shift .. + spread - 1
        (include/ieache.h section 3e).  spread=1, shift=0: bit p at coefficient p; tools.lut_pack_layout gives the placement of
        a table for pbs(..., tlwe=True)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if m is None:
            if rows.ndim < 2:
                raise ValueError("pack: rows must be [groups][m][n+1] or [m][n+1]")
            m = rows.shape[-2]
        m = int(m)
        rows = rows.reshape(-1, self.params.n + 1)
        if m >= 1 and rows.shape[0] % m:
            raise ValueError("pack: %d rows are no whole number of groups of %d" % (rows.shape[0], m))
        groups = rows.shape[0] // m if m >= 1 else 0
        out = np.zeros((groups, 2, self.params.N), dtype=np.int32)
        check(lib().ieache_pack(self.h, groups, m, int(spread), int(shift), _i32(rows), _i32(out), _stats_ref(stats)))
        return out

    def pack_plan(self, groups, m):
        """How pack() would cut such a call under the options as they are (csrc/pack_plan.h): dict(pieces, groups_per_piece,
        k_split, k_steps)."""
        out = (C.c_int64 * 4)()
        check(lib().ieache_debug_pack_plan(self.h, groups, int(m), out))
        return dict(zip(("pieces", "groups_per_piece", "k_split", "k_steps"), (int(v) for v in out)))

    def pack_device(self, groups, m, spread, shift, d_rows, d_out, stats=None):
        """Device pointers (ints): d_rows [groups m] rows of lwe_stride, d_out [groups][2][N] packed."""
        check(lib().ieache_pack_device(self.h, groups, int(m), int(spread), int(shift), C.c_void_p(d_rows), C.c_void_p(d_out), _stats_ref(stats)))

    def set_projection_key(self, pk, t=8, basebit=2):
        """The projection key [N][t][2][N] (tools.projection_keygen) for tlwe_project() and lut_write_coef(): replaces an earlier
        one; pk=None drops it.  Independent of the packing key."""
        if pk is None:
            check(lib().ieache_ctx_set_projection_key(self.h, 0, 0, None))
            return
        pk = np.ascontiguousarray(pk, dtype=np.int32)
        if int(t) >= 1 and pk.size != self.params.N * int(t) * 2 * self.params.N:  # (t < 1: the library refuses it)
            raise ValueError("projection key: expected [N][t][2][N] = %d words, got %d" % (self.params.N * t * 2 * self.params.N, pk.size))
        check(lib().ieache_ctx_set_projection_key(self.h, int(t), int(basebit), _i32(pk)))

    def tlwe_project(self, tlwe, first=0, width=1, dest=0, stats=None):
        """The projection on host rows (include/ieache.h section 3l): TLWE samples [count][2][N] (or one [2][N]) -> samples
        [count][2][N] that carry the phase of coefficients first .. first + width - 1 at dest .. (negacyclic, dest in [0, 2N))
        and zero elsewhere, plus the key switch's noise."""
        tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, self.params.N)
        out = np.zeros_like(tlwe)
        check(lib().ieache_tlwe_project(self.h, tlwe.shape[0], int(first), int(width), int(dest), _i32(tlwe), _i32(out), _stats_ref(stats)))
        return out

    def tlwe_project_device(self, count, first, width, dest, d_in, d_out, stats=None):
        """Device pointers (ints): d_in and d_out [count][2][N] packed; no overlap of the two is accepted."""
        check(lib().ieache_tlwe_project_device(self.h, count, int(first), int(width), int(dest), C.c_void_p(d_in), C.c_void_p(d_out), _stats_ref(stats)))

    def project_plan(self, count, width):
        """How tlwe_project() would cut such a call under the options as they are (csrc/project_plan.h): dict(pieces,
        items_per_piece, k_split, k_steps)."""
        out = (C.c_int64 * 4)()
        check(lib().ieache_debug_project_plan(self.h, count, int(width), out))
        return dict(zip(("pieces", "items_per_piece", "k_split", "k_steps"), (int(v) for v in out)))

    def lut_write_coef(self, tgsw, mem, depth, steps, new, width=1, unit=None, sel_of=None, stats=None):
        """The replace write of a window on host arrays (include/ieache.h section 3l):
        mem[i][hi_i].coef[lo_i unit .. lo_i unit + width) := new[i].coef[0 .. width).  mem [count][2^depth][2][N], new [count][2][N]
        with nothing outside its first `width` coefficients; sel_of [count][steps + depth], the `steps` LOW address bits first
        (None: samples i (steps + depth) + t mod n); unit defaults to width; width <= unit, unit 2^steps <= N -> the new memory."""
        depth, steps, width = int(depth), int(steps), int(width)
        unit = width if unit is None else int(unit)
        mem = np.ascontiguousarray(mem, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
        new = np.ascontiguousarray(new, dtype=np.int32).reshape(-1, 2, self.params.N)
        count = mem.shape[0]
        of = _opt_i32(sel_of, -1, max(depth + steps, 1))
        assert new.shape[0] == count and (of is None or depth + steps < 1 or of.shape[0] == count)
        out = np.zeros_like(mem)
        check(lib().ieache_lut_write_coef(self.h, tgsw.h, count, depth, steps, width, unit, _opt(of), _i32(new), _i32(mem), _i32(out),
                                          _stats_ref(stats)))
        return out

    def lut_write_coef_device(self, tgsw, count, depth, steps, width, unit, d_sel_of, d_new, d_mem, d_out, stats=None):
        """Device pointers (ints; d_sel_of may be None / 0): new [count][2][N], mem and out [count][2^depth][2][N] packed;
        d_out == d_mem writes in place."""
        check(lib().ieache_lut_write_coef_device(self.h, tgsw.h, count, int(depth), int(steps), int(width), int(unit), _dev(d_sel_of),
                                                 C.c_void_p(d_new), C.c_void_p(d_mem), C.c_void_p(d_out), _stats_ref(stats)))

    def unpack(self, tlwe, first=0, width=1, spread=1, keyswitch=True, stats=None):
        """The unpacking key switch on host rows (include/ieache.h section 3m), the partner of pack(): coefficients
        first + q spread, q < width, of TLWE samples [count][2][N] (or one [2][N]) -> LWE rows [count][width][n+1] under the gate
        key (keyswitch=False: the extracted rows [count][width][N+1]).  unpack(first=shift, spread=spread) reads back what
        pack(spread=spread, shift=shift) placed."""
        tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, self.params.N)
        out = np.zeros((tlwe.shape[0], max(int(width), 0), (self.params.n if keyswitch else self.params.N) + 1), dtype=np.int32)
        check(lib().ieache_unpack(self.h, tlwe.shape[0], int(first), int(width), int(spread), _i32(tlwe), 0 if keyswitch else UNPACK_NO_KEYSWITCH,
                                  _i32(out), _stats_ref(stats)))
        return out

    def unpack_device(self, count, first, width, spread, d_in, d_out, keyswitch=True, stats=None):
        """Device pointers (ints): d_in [count][2][N] packed, d_out [count][width] rows of lwe_stride words (keyswitch=False: of
        extract_stride words); no overlap of the two is accepted."""
        check(lib().ieache_unpack_device(self.h, count, int(first), int(width), int(spread), C.c_void_p(d_in), 0 if keyswitch else UNPACK_NO_KEYSWITCH,
                                         C.c_void_p(d_out), _stats_ref(stats)))

    def word_read(self, tgsw, tables, depth, steps, width=1, unit=None, sel_of=None, table_of=None, keyswitch=True, count=None, stats=None):
        """The read of an addressed word on host rows (section 3m), the partner of lut_write_coef():
        out[i][q] = LWE row of tables[table_of[i]][hi_i].coef[lo_i unit + q], q < width.  tables [n_tables][2^depth][2][N]; sel_of
        [count][steps + depth], the `steps` LOW address bits first (None: samples i (steps + depth) + t mod n); unit defaults to
        width; width <= unit, unit 2^steps <= N -> [count][width][n+1] (keyswitch=False: [count][width][N+1])."""
        depth, steps, width = int(depth), int(steps), int(width)
        unit = width if unit is None else int(unit)
        tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, self.params.N)
        of = _opt_i32(sel_of, -1, max(depth + steps, 1))
        tof = _opt_i32(table_of, -1)
        if count is None:
            count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth + steps > 0 else 1)
        assert (tof is None or tof.shape[0] == count) and (of is None or depth + steps < 1 or of.shape[0] == count)
        out = np.zeros((count, max(width, 0), (self.params.n if keyswitch else self.params.N) + 1), dtype=np.int32)
        check(lib().ieache_word_read(self.h, tgsw.h, count, depth, steps, width, unit, _opt(of), _i32(tables), tables.shape[0], _opt(tof),
                                     0 if keyswitch else UNPACK_NO_KEYSWITCH, _i32(out), _stats_ref(stats)))
        return out

    def word_read_device(self, tgsw, count, depth, steps, width, unit, d_sel_of, d_tables, n_tables, d_table_of, d_out, keyswitch=True, stats=None):
        """Device pointers (ints; the index arrays may be None / 0): tables [n_tables][2^depth][2][N] packed, out [count][width] rows
        of lwe_stride words (keyswitch=False: of extract_stride words)."""
        check(lib().ieache_word_read_device(self.h, tgsw.h, count, int(depth), int(steps), int(width), int(unit), _dev(d_sel_of), C.c_void_p(d_tables),
                                            int(n_tables), _dev(d_table_of), 0 if keyswitch else UNPACK_NO_KEYSWITCH, C.c_void_p(d_out),
                                            _stats_ref(stats)))

    def pbs_multi(self, x, test_polys, factors, poly_of=None, bias=None, keyswitch=True, stats=None, tlwe=False):
        """Multi-output programmable bootstrap on host rows: ONE blind rotation per row of x [count][n+1], as pbs does it, and
        one output per factor polynomial of factors [n_factors][N] (or one [N]): coefficient 0 of factor x accumulator,
        negacyclic and mod 2^32, plus bias[t] (None: 0) on its b term (include/ieache.h; tools.lut_factor_poly builds a factor
        from a table of small integers) -> [count][n_factors][n+1], or with keyswitch=False the extracted samples
        [count][n_factors][N+1] under the ring key.  The factor 1 gives pbs's own output.  tlwe=True: as for pbs."""
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.params.n + 1)
        tv = _pbs_table(self.params, test_polys, tlwe)
        fa = np.ascontiguousarray(factors, dtype=np.int32).reshape(-1, self.params.N)
        of = None if poly_of is None else np.ascontiguousarray(poly_of, dtype=np.int32).reshape(-1)
        bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.int32).reshape(-1)
        assert of is None or of.shape[0] == x.shape[0]
        assert bi is None or bi.shape[0] == fa.shape[0]
        out = np.zeros((x.shape[0], fa.shape[0], (self.params.n if keyswitch else self.params.N) + 1), dtype=np.int32)
        check(lib().ieache_pbs_multi(self.h, x.shape[0], _i32(x), _i32(tv), tv.shape[0], None if of is None else _i32(of), _i32(fa),
                                     fa.shape[0], None if bi is None else _i32(bi), _i32(out), _pbs_flags(keyswitch, tlwe), _stats_ref(stats)))
        return out

    def pbs_multi_device(self, count, d_x, d_test_polys, n_polys, d_poly_of, d_factors, n_factors, d_bias, d_out, keyswitch=True, stats=None,
                         tlwe=False):
        """Device pointers (ints; d_poly_of and d_bias may be None / 0): x rows of lwe_stride, test polynomials [n_polys][N] and
        factors [n_factors][N] packed, out [count * n_factors] rows of lwe_stride or, with keyswitch=False, of extract_stride."""
        check(lib().ieache_pbs_multi_device(self.h, count, C.c_void_p(d_x), C.c_void_p(d_test_polys), int(n_polys),
                                            C.c_void_p(d_poly_of or None), C.c_void_p(d_factors), int(n_factors), C.c_void_p(d_bias or None),
                                            C.c_void_p(d_out), _pbs_flags(keyswitch, tlwe), _stats_ref(stats)))

    def mux(self, a, b, c, stats=None):
        """bootsMUX on host rows: out[i] = a[i] ? b[i] : c[i]."""
        a, b, c = (np.ascontiguousarray(v, dtype=np.int32) for v in (a, b, c))
        assert a.shape == b.shape == c.shape and a.shape[-1] == self.params.n + 1
        out = np.zeros_like(a)
        check(lib().ieache_mux(self.h, a.size // (self.params.n + 1), _i32(a), _i32(b), _i32(c), _i32(out), _stats_ref(stats)))
        return out

    def mux_device(self, count, d_a, d_b, d_c, d_out, stats=None):
        check(lib().ieache_mux_device(self.h, count, C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c), C.c_void_p(d_out), _stats_ref(stats)))

    def debug_blind_rotate(self, x, steps=-1):
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.params.n + 1)
        acc = np.zeros((x.shape[0], 2, self.params.N), dtype=np.int32)
        check(lib().ieache_debug_blind_rotate(self.h, x.shape[0], _i32(x), _i32(acc), steps))
        return acc

    def debug_keyswitch(self, u):
        u = np.ascontiguousarray(u, dtype=np.int32).reshape(-1, self.params.N + 1)
        out = np.zeros((u.shape[0], self.params.n + 1), dtype=np.int32)
        check(lib().ieache_debug_keyswitch(self.h, u.shape[0], _i32(u), _i32(out)))
        return out

    # ---- the transform probe (csrc/fft_probe.h; include/ieache.h states the shapes) ----
    def debug_twiddles(self, which):
        """The 576-entry twiddle table as complex128: of the blind rotation (0), of the CMux family (1), as a 64-thread kernel
        builds it (2)."""
        out = np.zeros((TWIDDLE_ENTRIES, 2), dtype=np.float64)
        check(lib().ieache_debug_twiddles(self.h, which, _f64(out)))
        return out.view(np.complex128)[:, 0]

    def debug_fft512(self, form, x):
        """x [count][512] complex (forward forms: natural order; inverse forms: [count][8][64] flattened) -> complex128
        [count][8][64], raw in (register, lane) order."""
        x = np.ascontiguousarray(x, dtype=np.complex128).reshape(-1, 512)
        out = np.zeros((x.shape[0], 8, 64), dtype=np.complex128)
        check(lib().ieache_debug_fft512(self.h, form, x.shape[0], _f64(x.view(np.float64)), _f64(out.view(np.float64))))
        return out

    def debug_spectrum(self, which, first, count):
        """`count` prepared key polynomials from polynomial `first` on, complex128: [count][2][8][64] (which = 0, two-limb),
        [count][8][64] (1, one-limb) or [count][2][N/2] (2, the any-parameter kernel's bit-reversed order)."""
        shape = {0: (count, 2, 8, 64), 1: (count, 8, 64)}.get(which, (count, 2, self.params.N // 2))
        out = np.zeros(shape, dtype=np.complex128)
        check(lib().ieache_debug_spectrum(self.h, which, first, count, _f64(out.view(np.float64))))
        return out


class _MemberContext(Context):
    """A member of a Group as a Context (ieache_group_ctx): borrowed -- closing it only forgets the handle, the group destroys it."""

    def close(self):
        self.h = None

    __del__ = close


class _MemberStats:
    """The stats= argument of a Group call: the ieache_stats array the call fills, handed back as one Stats per member."""

    def __init__(self, stats, members):
        self.into = stats
        self.array = (Stats * members)() if stats is not None else None

    @property
    def ref(self):
        return self.array  # None: a null pointer

    def deliver(self):
        if self.into is not None:
            self.into[:] = [Stats.from_buffer_copy(s) for s in self.array]


class Group:
    """The cloud key resident on several GPUs behind one handle (ieache_group): every host-buffer call of Context, cut into
    contiguous slices of rows or expressions, one per member, evaluated side by side on host threads of the library.

        with Group.from_file("cloud.key", range(device_count())) as g:
            out = g.eval_batch(CIRC_ADD, 32, in_lwe)

    Outputs equal a Context's word for word.  A device may be listed more than once (several contexts on one card); such
    members start with option "br_mix" = 0 (include/ieache.h, section 2b).  One call at a time: not thread-safe.  Every
    method takes stats=: a list the call fills with one Stats per member (all zero for a member whose slice was empty)."""

    def __init__(self, handle):
        if not handle:
            msg = lib().ieache_last_error().decode()
            # a NULL handle carries no code: a member that could not be made is named first, everything else is an argument
            raise IeacheError(-19 if msg.startswith("member ") else -22, msg)
        self.h = handle
        n = check(lib().ieache_group_size(self.h))
        self.devices = tuple(check(lib().ieache_group_device(self.h, m)) for m in range(n))
        # borrowed views: they do not destroy, and lose their handle when the group closes
        self.contexts = tuple(_MemberContext(lib().ieache_group_ctx(self.h, m)) for m in range(n))
        self.params = self.contexts[0].params
        self._fold = False

    @staticmethod
    def _device_list(devices):
        devices = [int(d) for d in devices]
        return (C.c_int * max(len(devices), 1))(*devices), len(devices)

    @classmethod
    def from_file(cls, cloud_key_path, devices):
        arr, n = cls._device_list(devices)
        return cls(lib().ieache_group_create(os.fsencode(cloud_key_path), arr, n))

    @classmethod
    def from_arrays(cls, params, bk, ksk, devices):
        bk = np.ascontiguousarray(bk, dtype=np.int32)
        ksk = np.ascontiguousarray(ksk, dtype=np.int32)
        assert bk.size == params.bk_count and ksk.size == params.ksk_count
        arr, n = cls._device_list(devices)
        return cls(lib().ieache_group_create_raw(C.byref(params), _i32(bk), _i32(ksk), arr, n))

    def close(self):
        if getattr(self, "h", None):
            for c in self.contexts:
                c.close()
            lib().ieache_group_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return len(self.devices)

    def set_option(self, name, value):
        """Context.set_option on every member, all or none: a value any member refuses raises and changes no member."""
        check(lib().ieache_group_set_option(self.h, name.encode(), int(value)))
        if name == "fold_constants":
            self._fold = bool(value)
            for c in self.contexts:
                c._fold = bool(value)

    def _rows(self, *arrays):
        arrays = [np.ascontiguousarray(v, dtype=np.int32) for v in arrays]
        assert all(v.shape == arrays[0].shape for v in arrays) and arrays[0].shape[-1] == self.params.n + 1
        return arrays, arrays[0].size // (self.params.n + 1)

    def prepare(self, kind, bits, batch):
        """Context.prepare on every member, each for its slice of `batch` expressions."""
        check(lib().ieache_group_prepare_batch(self.h, kind, bits, batch))

    def prepare_netlist(self, nl, batch):
        check(lib().ieache_group_prepare_netlist(self.h, nl.h, batch))

    def eval_batch(self, kind, bits, in_lwe, stats=None):
        """in_lwe [batch][n_inputs][n+1] int32 on the host -> [batch][n_outputs][n+1], as Context.eval_batch."""
        info = circuit_info(kind, bits, self._fold)
        in_lwe = np.ascontiguousarray(in_lwe, dtype=np.int32)
        batch = in_lwe.shape[0]
        assert in_lwe.shape == (batch, info.n_inputs, self.params.n + 1), in_lwe.shape
        out = np.zeros((batch, info.n_outputs, self.params.n + 1), dtype=np.int32)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_eval_batch(self.h, kind, bits, batch, _i32(in_lwe), _i32(out), st.ref))
        st.deliver()
        return out

    def eval_netlist(self, nl, in_lwe, stats=None):
        """One CompiledNetlist, read by every member, over a batch: as Context.eval_netlist."""
        info = nl.info()
        in_lwe = np.ascontiguousarray(in_lwe, dtype=np.int32)
        batch = in_lwe.shape[0]
        assert in_lwe.shape == (batch, info.n_inputs, self.params.n + 1), in_lwe.shape
        out = np.zeros((batch, info.n_outputs, self.params.n + 1), dtype=np.int32)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_eval_netlist(self.h, nl.h, batch, _i32(in_lwe), _i32(out), st.ref))
        st.deliver()
        return out

    def eval_jobs(self, jobs, stats=None):
        """Context.eval_jobs with every job's batch cut over the members (ieache_shard_slice)."""
        jobs = list(jobs)
        arr, _ins, outs = _job_array(jobs, self.params.n + 1, self._fold)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_eval_jobs(self.h, arr, len(jobs), st.ref))
        st.deliver()
        return outs

    def gates(self, gate_type, a, b, stats=None):
        (a, b), count = self._rows(a, b)
        out = np.zeros_like(a)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_gates(self.h, gate_type, count, _i32(a), _i32(b), _i32(out), st.ref))
        st.deliver()
        return out

    def gates3(self, gate_type, a, b, c, stats=None):
        (a, b, c), count = self._rows(a, b, c)
        out = np.zeros_like(a)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_gates3(self.h, gate_type, count, _i32(a), _i32(b), _i32(c), _i32(out), st.ref))
        st.deliver()
        return out

    def mux(self, a, b, c, stats=None):
        (a, b, c), count = self._rows(a, b, c)
        out = np.zeros_like(a)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_mux(self.h, count, _i32(a), _i32(b), _i32(c), _i32(out), st.ref))
        st.deliver()
        return out

    def pbs(self, x, test_polys, poly_of=None, keyswitch=True, stats=None, tlwe=False, accumulator=False):
        """Context.pbs: the test polynomials go to every member whole, poly_of is cut with the rows."""
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.params.n + 1)
        tv = _pbs_table(self.params, test_polys, tlwe)
        of = None if poly_of is None else np.ascontiguousarray(poly_of, dtype=np.int32).reshape(-1)
        assert of is None or of.shape[0] == x.shape[0]
        out = _pbs_out(self.params, x.shape[0], keyswitch, accumulator)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_pbs(self.h, x.shape[0], _i32(x), _i32(tv), tv.shape[0], None if of is None else _i32(of), _i32(out),
                                     _pbs_flags(keyswitch, tlwe, accumulator), st.ref))
        st.deliver()
        return out

    def pbs_multi(self, x, test_polys, factors, poly_of=None, bias=None, keyswitch=True, stats=None, tlwe=False):
        """Context.pbs_multi: test polynomials, factors and bias go to every member whole -> [count][n_factors][rows]."""
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.params.n + 1)
        tv = _pbs_table(self.params, test_polys, tlwe)
        fa = np.ascontiguousarray(factors, dtype=np.int32).reshape(-1, self.params.N)
        of = None if poly_of is None else np.ascontiguousarray(poly_of, dtype=np.int32).reshape(-1)
        bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.int32).reshape(-1)
        assert of is None or of.shape[0] == x.shape[0]
        assert bi is None or bi.shape[0] == fa.shape[0]
        out = np.zeros((x.shape[0], fa.shape[0], (self.params.n if keyswitch else self.params.N) + 1), dtype=np.int32)
        st = _MemberStats(stats, len(self))
        check(lib().ieache_group_pbs_multi(self.h, x.shape[0], _i32(x), _i32(tv), tv.shape[0], None if of is None else _i32(of), _i32(fa),
                                           fa.shape[0], None if bi is None else _i32(bi), _i32(out), _pbs_flags(keyswitch, tlwe), st.ref))
        st.deliver()
        return out
