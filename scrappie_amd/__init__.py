"""scrappie_amd -- Python host side over libscrappie_hip.so (the MI355X-native
`scrappie raw` hot path).

It mirrors the reference's `scrappy` binding (python/scrappy/__init__.py:47-430:
RawTable, ScrappyMatrix, calc_post, decode_post, basecall_raw, get_model_stride)
so code and tests written against `scrappy` read the same, and adds the batched
`Engine`, which is the fast path.  Bindings are plain ctypes over the C ABI in
include/scrappie_hip.h -- no torch types cross the boundary.

The HIP library is required: importing the compute entry points without
scrappie_amd/libscrappie_hip.so raises (there is no CPU fallback).
"""
import ctypes as C
import os
import sys
import subprocess

import numpy as np

from . import model as _model

__version__ = "0.1.0"
_HERE = os.path.dirname(os.path.abspath(__file__))
# the experiments build (kernel forms measured and not adopted, cycle stamps: make -C csrc ../libscrappie_hip_exp.so) is loaded only when
# SCRAPPIE_HIP_LIB names it -- the tests of those forms do, in processes of their own
EXP_LIB_PATH = os.path.join(_HERE, "libscrappie_hip_exp.so")
LIB_PATH = os.environ.get("SCRAPPIE_HIP_LIB") or os.path.join(_HERE, "libscrappie_hip.so")

ftype = np.float32
vsize = 4


class _Mat(C.Structure):
    _fields_ = [("nr", C.c_size_t), ("nrq", C.c_size_t), ("nc", C.c_size_t),
                ("stride", C.c_size_t), ("data", C.c_void_p)]


class _RawTable(C.Structure):
    _fields_ = [("uuid", C.c_char_p), ("n", C.c_size_t), ("start", C.c_size_t),
                ("end", C.c_size_t), ("raw", C.POINTER(C.c_float))]


class Params(C.Structure):
    """scrappie_hip_params; defaults are the CLI's (src/scrappie_raw.c:98-121)."""
    _fields_ = [("min_prob", C.c_float), ("tempW", C.c_float), ("tempb", C.c_float),
                ("stay_pen", C.c_float), ("skip_pen", C.c_float), ("local_pen", C.c_float),
                ("use_slip", C.c_int), ("homopolymer", C.c_int), ("want_pos", C.c_int)]


class _Call(C.Structure):
    _fields_ = [("score", C.c_float), ("nblock", C.c_size_t), ("basecall", C.c_void_p),
                ("basecall_length", C.c_size_t), ("pos", C.POINTER(C.c_int))]


class _MapTarget(C.Structure):
    _fields_ = [("seq", C.POINTER(C.c_int)), ("seqlen", C.c_size_t), ("poslow", C.POINTER(C.c_size_t)),
                ("poshigh", C.POINTER(C.c_size_t))]


class _MapResult(C.Structure):
    _fields_ = [("score", C.c_float), ("nblock", C.c_size_t), ("path", C.POINTER(C.c_int32))]


class _MapLocalTarget(C.Structure):
    _fields_ = [("seq", C.POINTER(C.c_int)), ("seqlen", C.c_size_t)]


class _MapLocalResult(C.Structure):
    _fields_ = [("score", C.c_float), ("nblock", C.c_size_t), ("first", C.c_size_t), ("last", C.c_size_t),
                ("path", C.POINTER(C.c_int32))]


class _FindResult(C.Structure):
    _fields_ = [("score", C.POINTER(C.c_float)), ("begin", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("nmotif", C.c_size_t), ("call_score", C.c_float), ("best", C.c_int), ("nblock", C.c_size_t)]


class _EditsResult(C.Structure):
    _fields_ = [("base", C.c_float), ("sub", C.POINTER(C.c_float)), ("dele", C.POINTER(C.c_float)), ("ins", C.POINTER(C.c_float)),
                ("seqlen", C.c_size_t), ("nblock", C.c_size_t)]


class _MapCandidates(C.Structure):
    _fields_ = [("cand", C.POINTER(_MapTarget)), ("ncand", C.c_size_t)]


class _MapMultiResult(C.Structure):
    _fields_ = [("score", C.POINTER(C.c_float)), ("ncand", C.c_size_t), ("best", C.c_int), ("nblock", C.c_size_t),
                ("path", C.POINTER(C.c_int32))]


class _SquigTarget(C.Structure):
    _fields_ = [("params", C.POINTER(C.c_float)), ("npos", C.c_size_t), ("stride", C.c_size_t)]


class _SquigParams(C.Structure):
    _fields_ = [("rate", C.c_float), ("prob_back", C.c_float), ("local_pen", C.c_float), ("skip_pen", C.c_float),
                ("minscore", C.c_float)]


class _SquigBand(C.Structure):
    _fields_ = [("low", C.POINTER(C.c_int32)), ("width", C.c_size_t)]


class _SquigResult(C.Structure):
    _fields_ = [("score", C.c_float), ("n", C.c_size_t), ("path", C.POINTER(C.c_int32))]


class _SquigLocalResult(C.Structure):
    _fields_ = [("score", C.c_float), ("first", C.c_size_t), ("last", C.c_size_t), ("n", C.c_size_t), ("path", C.POINTER(C.c_int32))]


class _SquigCandidates(C.Structure):
    _fields_ = [("cand", C.POINTER(_SquigTarget)), ("ncand", C.c_size_t)]


class _SquigMultiResult(C.Structure):
    _fields_ = [("score", C.POINTER(C.c_float)), ("ncand", C.c_size_t), ("best", C.c_int), ("n", C.c_size_t),
                ("path", C.POINTER(C.c_int32))]


class _Event(C.Structure):          # scrappie_structures.h:8-15
    _fields_ = [("start", C.c_uint64), ("length", C.c_float), ("mean", C.c_float), ("stdv", C.c_float),
                ("pos", C.c_int), ("state", C.c_int)]


class _EventTable(C.Structure):     # scrappie_structures.h:17-22
    _fields_ = [("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t), ("event", C.POINTER(_Event))]


class DetectorParam(C.Structure):   # event_detection.h:6-12; the defaults are event_detection_defaults
    _fields_ = [("window_length1", C.c_size_t), ("window_length2", C.c_size_t), ("threshold1", C.c_float),
                ("threshold2", C.c_float), ("peak_height", C.c_float)]

    def __init__(self, window_length1=3, window_length2=6, threshold1=1.4, threshold2=9.0, peak_height=0.2):
        super().__init__(window_length1, window_length2, threshold1, threshold2, peak_height)


class DwellModel(C.Structure):      # decode.h:8-11
    _fields_ = [("scale", C.c_float), ("base_adj", C.c_float * 4)]


class _EventResult(C.Structure):
    _fields_ = [("events", _EventTable), ("status", C.c_int)]


class Timing(C.Structure):
    _fields_ = [("conv_ms", C.c_float), ("affine_ms", C.c_float), ("gru_ms", C.c_float),
                ("ff_ms", C.c_float), ("decode_ms", C.c_float), ("backtrace_ms", C.c_float),
                ("total_ms", C.c_float), ("n_gru_launches", C.c_int), ("n_affine_launches", C.c_int),
                ("gru_flops", C.c_double), ("affine_flops", C.c_double), ("ff_flops", C.c_double),
                ("fused_ms", C.c_float), ("n_fused_launches", C.c_int), ("fused_flops", C.c_double),
                ("stitch_ms", C.c_float)]


def build(verbose=False):
    """Compile libscrappie_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "../libscrappie_hip.so"], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)


_lib = None


def _one_hip_runtime():
    """A process must hold ONE HIP runtime: a second copy finds no device once the first has initialised
    (hipGetDeviceCount: "no ROCm-capable device is detected").  torch wheels bundle their own copy (torch/lib/libamdhip64.so) and ask
    for it as "libamdhip64.so", which does not match the soname (libamdhip64.so.7) of a copy libscrappie_hip.so brought in from
    /opt/rocm/lib earlier -- so `import scrappie_amd; ...; import torch` used to end with two.  Loading torch's copy first (when a torch
    is installed and not imported yet) makes this library bind to it by soname and torch find it again by file: one runtime whatever the
    import order.  SCRAPPIE_HIP_SYSTEM_RUNTIME=1 keeps /opt/rocm's (then import torch BEFORE this library, or not at all)."""
    import importlib.util
    if "torch" in sys.modules or os.environ.get("SCRAPPIE_HIP_SYSTEM_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    """The loaded C library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(scrappie_amd has no CPU fallback)" % LIB_PATH)
    # an engine's four streams want a hardware queue each (scrappie_hip.hip: hw_queue_default); effective only if HIP
    # has not initialised in this process yet -- with torch imported first, set GPU_MAX_HW_QUEUES before importing it
    if not os.environ.get("SH_NO_PY_QUEUE_DEFAULT"):        # (switch for checking the C side's own default)
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
    PM = C.POINTER(_Mat)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.scrappie_hip_last_error.restype = C.c_char_p
    L.scrappie_hip_device_count.restype = C.c_int
    L.scrappie_hip_engine_create.restype = C.c_void_p
    L.scrappie_hip_engine_create.argtypes = [C.c_int]
    L.scrappie_hip_engine_destroy.argtypes = [C.c_void_p]
    L.scrappie_hip_default_params.restype = Params
    L.scrappie_hip_load_model.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.scrappie_hip_load_model_mem.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    L.scrappie_hip_find_model.argtypes = [C.c_void_p, C.c_char_p]
    L.scrappie_hip_register_model.argtypes = [C.c_char_p, C.c_char_p]
    L.scrappie_hip_basecall_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.c_size_t,
                                              C.POINTER(Params), C.POINTER(_Call)]
    L.scrappie_hip_basecall_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(Params),
                                               C.POINTER(_Call)]
    L.scrappie_hip_run_device.restype = C.c_long
    L.scrappie_hip_run_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(Params)]
    L.scrappie_hip_collect.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(_Call), C.c_size_t]
    L.scrappie_hip_free_calls.argtypes = [C.POINTER(_Call), C.c_size_t]
    L.scrappie_hip_basecall_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_size_t, C.POINTER(_RawTable),
                                                    C.c_size_t, C.POINTER(Params), C.POINTER(_Call)]
    L.scrappie_hip_plan_dynamic.restype = C.c_long
    L.scrappie_hip_plan_dynamic.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.c_size_t]
    L.scrappie_hip_set_decoder_input.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
    L.scrappie_hip_set_trunk_input.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
    L.scrappie_hip_debug_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.scrappie_hip_debug_fetch.restype = C.c_longlong
    L.scrappie_hip_debug_fetch.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    L.scrappie_hip_debug_stitch.restype = C.c_long
    L.scrappie_hip_debug_stitch.argtypes = [C.c_void_p, ip, fp, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t, ip, ip]
    L.scrappie_hip_posterior.restype = PM
    L.scrappie_hip_posterior.argtypes = [C.c_void_p, C.c_int, _RawTable, C.c_float, C.c_float, C.c_float, C.c_bool]
    L.scrappie_hip_trunk.restype = PM
    L.scrappie_hip_trunk.argtypes = [C.c_void_p, C.c_int, _RawTable, C.c_int]
    L.scrappie_hip_min_samples.restype = C.c_size_t
    L.scrappie_hip_min_samples.argtypes = [C.c_void_p, C.c_int]
    L.scrappie_hip_model_stride.argtypes = [C.c_void_p, C.c_int]
    L.scrappie_hip_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.scrappie_hip_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.scrappie_hip_set_max_launch_reads.argtypes = [C.c_void_p, C.c_size_t]
    L.scrappie_hip_set_max_launch_blocks.argtypes = [C.c_void_p, C.c_size_t]
    L.scrappie_hip_plan_groups.restype = C.c_long
    L.scrappie_hip_plan_groups.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_size_t, C.c_size_t,
                                           C.POINTER(C.c_size_t), C.c_size_t]
    L.scrappie_hip_device_alloc.restype = C.c_void_p
    L.scrappie_hip_device_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.scrappie_hip_device_free.argtypes = [C.c_void_p, C.c_void_p]
    L.scrappie_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.scrappie_hip_synchronize.argtypes = [C.c_void_p]
    L.scrappie_hip_format_fasta.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p,
                                            C.POINTER(_Call), C.c_size_t, C.c_size_t, C.c_size_t]
    # per-read reference surface (python/pyscrap.h)
    for nm in ("nanonet_raw_posterior", "nanonet_rgrgr_r94_posterior", "nanonet_rgrgr_r941_posterior", "nanonet_rgrgr_r10_posterior",
               "nanonet_rnnrf_r94_transitions"):
        getattr(L, nm).restype = PM
        getattr(L, nm).argtypes = [_RawTable, C.c_float, C.c_float, C.c_float, C.c_bool]
    L.decode_transducer.restype = C.c_float
    L.decode_transducer.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_bool]
    L.overlapper.restype = C.c_void_p
    L.overlapper.argtypes = [ip, C.c_size_t, C.c_int, ip]
    L.decode_crf.restype = C.c_float
    L.decode_crf.argtypes = [PM, ip]
    L.crfpath_to_basecall.restype = C.c_void_p
    L.crfpath_to_basecall.argtypes = [ip, C.c_size_t, ip]
    L.posterior_crf.restype = PM
    L.posterior_crf.argtypes = [PM]
    L.homopolymer_path.argtypes = [PM, ip, C.c_int]
    L.medmad_normalise_array.argtypes = [fp, C.c_size_t]
    L.trim_raw_by_mad.restype = _RawTable
    L.trim_raw_by_mad.argtypes = [_RawTable, C.c_size_t, C.c_float]
    L.trim_and_segment_raw.restype = _RawTable
    L.trim_and_segment_raw.argtypes = [_RawTable, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float]
    L.mat_from_array.restype = PM
    L.mat_from_array.argtypes = [fp, C.c_size_t, C.c_size_t]
    L.make_scrappie_matrix.restype = PM
    L.make_scrappie_matrix.argtypes = [C.c_size_t, C.c_size_t]
    L.free_scrappie_matrix.restype = PM
    L.free_scrappie_matrix.argtypes = [PM]
    L.scrappie_hip_prep_create.restype = C.c_void_p
    L.scrappie_hip_prep_create.argtypes = [C.c_int]
    L.scrappie_hip_prep_destroy.argtypes = [C.c_void_p]
    L.scrappie_hip_prep_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                        C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.scrappie_hip_prep_begin.restype = C.c_void_p
    L.scrappie_hip_prep_begin.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.scrappie_hip_prep_alloc.restype = C.c_void_p
    L.scrappie_hip_prep_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.scrappie_hip_prep_owns.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.scrappie_hip_prep_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, fp]
    L.scrappie_hip_prep_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    L.get_raw_model_stride_from_string.argtypes = [C.c_char_p]
    L.get_raw_model.argtypes = [C.c_char_p]
    sp = C.POINTER(C.c_size_t)
    L.are_bounds_sane.restype = C.c_bool
    L.are_bounds_sane.argtypes = [sp, sp, C.c_size_t, C.c_size_t]
    L.map_to_sequence_viterbi.restype = C.c_float
    L.map_to_sequence_viterbi.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, ip]
    L.map_to_sequence_forward.restype = C.c_float
    L.map_to_sequence_forward.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t]
    for nm in ("map_to_sequence_viterbi_banded", "map_to_sequence_forward_banded"):
        getattr(L, nm).restype = C.c_float
        getattr(L, nm).argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, sp, sp]
    L.map_crf_to_sequence_viterbi.restype = C.c_float
    L.map_crf_to_sequence_viterbi.argtypes = [PM, ip, C.c_size_t, ip]
    L.map_crf_to_sequence_forward.restype = C.c_float
    L.map_crf_to_sequence_forward.argtypes = [PM, ip, C.c_size_t]
    L.map_crf_to_sequence_viterbi_banded.restype = C.c_float
    L.map_crf_to_sequence_viterbi_banded.argtypes = [PM, ip, C.c_size_t, sp, sp, ip]
    L.map_crf_to_sequence_forward_banded.restype = C.c_float
    L.map_crf_to_sequence_forward_banded.argtypes = [PM, ip, C.c_size_t, sp, sp]
    L.scrappie_hip_map_crf_bounds_sane.argtypes = [sp, sp, C.c_size_t, C.c_size_t]
    L.scrappie_hip_map_crf_diagonal_band.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, sp, sp]
    L.scrappie_hip_map_crf_lds_max_seq.restype = C.c_size_t
    L.scrappie_hip_map_crf_lds_max_seq.argtypes = []
    L.scrappie_hip_map_crf_plan_scratch.restype = C.c_longlong
    L.scrappie_hip_map_crf_plan_scratch.argtypes = [sp, sp, C.c_size_t, C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_crf_form_counts.restype = None
    L.scrappie_hip_map_crf_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.map_crf_to_reference_viterbi.restype = C.c_float
    L.map_crf_to_reference_viterbi.argtypes = [PM, ip, C.c_size_t, sp, sp, ip]
    L.map_crf_to_reference_forward.restype = C.c_float
    L.map_crf_to_reference_forward.argtypes = [PM, ip, C.c_size_t]
    L.scrappie_hip_map_local_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapLocalTarget), C.c_size_t,
                                               C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_MapLocalResult)]
    L.scrappie_hip_free_map_local_results.restype = None
    L.scrappie_hip_free_map_local_results.argtypes = [C.POINTER(_MapLocalResult), C.c_size_t]
    L.scrappie_hip_map_crf_local_plan.restype = C.c_longlong
    L.scrappie_hip_map_crf_local_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_long, C.c_size_t, sp, sp, sp, ip, C.POINTER(C.c_longlong),
                                                  C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_crf_local_stride.restype = C.c_size_t
    L.scrappie_hip_map_crf_local_stride.argtypes = [C.c_size_t, C.c_size_t, C.c_long]
    L.scrappie_hip_map_crf_local_max_cells.restype = C.c_size_t
    L.scrappie_hip_map_crf_local_max_cells.argtypes = []
    L.scrappie_hip_map_crf_local_form_counts.restype = None
    L.scrappie_hip_map_crf_local_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.map_to_reference_viterbi.restype = C.c_float
    L.map_to_reference_viterbi.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, sp, sp, ip]
    L.map_to_reference_forward.restype = C.c_float
    L.map_to_reference_forward.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t]
    L.scrappie_hip_map_post_local_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapLocalTarget), C.c_size_t,
                                                    C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_MapLocalResult)]
    L.scrappie_hip_map_local_plan.restype = C.c_longlong
    L.scrappie_hip_map_local_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_long, C.c_size_t, sp, sp, sp, ip, C.POINTER(C.c_longlong),
                                              C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_local_stride.restype = C.c_size_t
    L.scrappie_hip_map_local_stride.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_long]
    L.scrappie_hip_map_local_max_cells.restype = C.c_size_t
    L.scrappie_hip_map_local_max_cells.argtypes = [C.c_size_t]
    L.scrappie_hip_map_local_form_counts.restype = None
    L.scrappie_hip_map_local_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_find_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapCandidates), C.c_size_t,
                                          C.POINTER(Params), C.c_int, C.POINTER(_FindResult)]
    L.scrappie_hip_free_find_results.restype = None
    L.scrappie_hip_free_find_results.argtypes = [C.POINTER(_FindResult), C.c_size_t]
    L.find_crf_sequences_viterbi.argtypes = [PM, C.POINTER(_MapTarget), C.c_size_t, fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), fp]
    L.scrappie_hip_crf_find_plan.restype = C.c_long
    L.scrappie_hip_crf_find_plan.argtypes = [sp, C.c_size_t, C.c_size_t, ip, C.POINTER(C.c_longlong)]
    L.scrappie_hip_crf_find_max_cells.restype = C.c_size_t
    L.scrappie_hip_crf_find_max_cells.argtypes = []
    L.scrappie_hip_crf_find_form_counts.restype = None
    L.scrappie_hip_crf_find_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.encode_bases_to_integers.restype = C.c_void_p
    L.encode_bases_to_integers.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
    L.scrappie_hip_read_blocks.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.scrappie_hip_model_states.argtypes = [C.c_void_p, C.c_int]
    L.scrappie_hip_map_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapTarget), C.c_size_t,
                                         C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_MapResult)]
    L.scrappie_hip_free_map_results.argtypes = [C.POINTER(_MapResult), C.c_size_t]
    L.scrappie_hip_map_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scrappie_hip_map_multi_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapCandidates), C.c_size_t,
                                               C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_MapMultiResult)]
    L.scrappie_hip_free_map_multi_results.restype = None
    L.scrappie_hip_free_map_multi_results.argtypes = [C.POINTER(_MapMultiResult), C.c_size_t]
    L.scrappie_hip_map_post_multi.argtypes = [PM, C.c_float, C.c_float, C.c_float, C.POINTER(_MapTarget), C.c_size_t, C.c_int, fp]
    L.scrappie_hip_map_pack_plan.restype = C.c_long
    L.scrappie_hip_map_pack_plan.argtypes = [sp, C.c_size_t, C.c_size_t, ip, C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_pack_max_cells.restype = C.c_size_t
    L.scrappie_hip_map_pack_max_cells.argtypes = []
    L.scrappie_hip_map_pack_form_counts.restype = None
    L.scrappie_hip_map_pack_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_map_crf_multi_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapCandidates), C.c_size_t,
                                                   C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_MapMultiResult)]
    L.scrappie_hip_map_trans_multi.argtypes = [PM, C.POINTER(_MapTarget), C.c_size_t, C.c_int, fp]
    L.scrappie_hip_map_crf_pack_plan.restype = C.c_long
    L.scrappie_hip_map_crf_pack_plan.argtypes = [sp, C.c_size_t, C.c_size_t, ip, C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_crf_pack_max_cells.restype = C.c_size_t
    L.scrappie_hip_map_crf_pack_max_cells.argtypes = []
    L.scrappie_hip_map_crf_pack_form_counts.restype = None
    L.scrappie_hip_map_crf_pack_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_map_crf_edits_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.POINTER(_MapTarget), C.c_size_t,
                                                   C.POINTER(Params), C.c_int, C.POINTER(_EditsResult)]
    L.scrappie_hip_free_edits_results.restype = None
    L.scrappie_hip_free_edits_results.argtypes = [C.POINTER(_EditsResult), C.c_size_t]
    L.map_crf_edits.argtypes = [PM, ip, C.c_size_t, C.c_int, fp, fp, fp, fp]
    L.scrappie_hip_crf_edits_pitch.restype = C.c_size_t
    L.scrappie_hip_crf_edits_pitch.argtypes = [C.c_size_t]
    L.scrappie_hip_crf_edits_row_bytes.restype = C.c_size_t
    L.scrappie_hip_crf_edits_row_bytes.argtypes = [C.c_size_t, C.c_size_t]
    L.scrappie_hip_crf_edits_plan.restype = C.c_longlong
    L.scrappie_hip_crf_edits_plan.argtypes = [sp, sp, C.c_size_t, ip, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_crf_edits_form_counts.restype = None
    L.scrappie_hip_crf_edits_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_crf_edits_timing.restype = None
    L.scrappie_hip_crf_edits_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), sp, sp]
    L.scrappie_hip_map_crf_edits_banded_batch.argtypes = L.scrappie_hip_map_crf_edits_batch.argtypes
    L.map_crf_edits_banded.argtypes = [PM, ip, C.c_size_t, sp, sp, C.c_int, fp, fp, fp, fp]
    L.scrappie_hip_map_crf_path_band.argtypes = [ip, C.c_size_t, C.c_size_t, C.c_size_t, sp, sp]
    L.scrappie_hip_crf_edits_band_pitch.restype = C.c_size_t
    L.scrappie_hip_crf_edits_band_pitch.argtypes = [sp, sp, C.c_size_t]
    L.scrappie_hip_crf_edits_band_row_bytes.restype = C.c_size_t
    L.scrappie_hip_crf_edits_band_row_bytes.argtypes = [sp, sp, C.c_size_t]
    L.scrappie_hip_crf_edits_band_plan.restype = C.c_longlong
    L.scrappie_hip_crf_edits_band_plan.argtypes = [sp, sp, C.POINTER(sp), C.POINTER(sp), C.c_size_t, ip, C.POINTER(C.c_longlong),
                                                   C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_crf_edits_band_form_counts.restype = None
    L.scrappie_hip_crf_edits_band_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_crf_edits_band_scratch.restype = None
    L.scrappie_hip_crf_edits_band_scratch.argtypes = [C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_edits_batch.argtypes = L.scrappie_hip_map_crf_edits_batch.argtypes
    L.map_post_edits.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, C.c_int, fp, fp, fp, fp]
    L.scrappie_hip_map_edits_banded_batch.argtypes = L.scrappie_hip_map_crf_edits_batch.argtypes
    L.map_post_edits_banded.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, sp, sp, C.c_int, fp, fp, fp, fp]
    L.scrappie_hip_map_path_band.argtypes = [ip, C.c_size_t, C.c_size_t, C.c_size_t, sp, sp]
    L.scrappie_hip_map_edits_band_pitch.restype = C.c_size_t
    L.scrappie_hip_map_edits_band_pitch.argtypes = [sp, sp, C.c_size_t]
    L.scrappie_hip_map_edits_band_row_bytes.restype = C.c_size_t
    L.scrappie_hip_map_edits_band_row_bytes.argtypes = [sp, sp, C.c_size_t]
    L.scrappie_hip_map_edits_band_plan.restype = C.c_longlong
    L.scrappie_hip_map_edits_band_plan.argtypes = [sp, sp, C.POINTER(sp), C.POINTER(sp), C.c_size_t, C.c_size_t, ip, C.POINTER(C.c_longlong),
                                                   C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_edits_band_form_counts.restype = None
    L.scrappie_hip_map_edits_band_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_map_edits_band_scratch.restype = None
    L.scrappie_hip_map_edits_band_scratch.argtypes = [C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_edits_pitch.restype = C.c_size_t
    L.scrappie_hip_map_edits_pitch.argtypes = [C.c_size_t, C.c_size_t]
    L.scrappie_hip_map_edits_row_bytes.restype = C.c_size_t
    L.scrappie_hip_map_edits_row_bytes.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t]
    L.scrappie_hip_map_edits_plan.restype = C.c_longlong
    L.scrappie_hip_map_edits_plan.argtypes = [sp, sp, C.c_size_t, C.c_size_t, ip, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_map_edits_max_bases.restype = C.c_size_t
    L.scrappie_hip_map_edits_max_bases.argtypes = [C.c_size_t]
    L.scrappie_hip_map_edits_form_counts.restype = None
    L.scrappie_hip_map_edits_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_map_edits_timing.restype = None
    L.scrappie_hip_map_edits_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), sp, sp]
    L.squiggle_match_viterbi.restype = C.c_float
    L.squiggle_match_viterbi.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int32)]
    L.squiggle_match_forward.restype = C.c_float
    L.squiggle_match_forward.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float]
    L.scrappie_hip_squiggle_match_batch.argtypes = [C.c_void_p, C.POINTER(_RawTable), C.POINTER(_SquigTarget), C.c_size_t,
                                                    C.POINTER(_SquigParams), C.c_int, C.c_int, C.POINTER(_SquigResult)]
    L.scrappie_hip_free_squiggle_results.argtypes = [C.POINTER(_SquigResult), C.c_size_t]
    i32p = C.POINTER(C.c_int32)
    L.squiggle_match_viterbi_banded.restype = C.c_float
    L.squiggle_match_viterbi_banded.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float, i32p, C.c_size_t, i32p]
    L.squiggle_match_forward_banded.restype = C.c_float
    L.squiggle_match_forward_banded.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float, i32p, C.c_size_t]
    L.scrappie_hip_squiggle_match_banded_batch.argtypes = [C.c_void_p, C.POINTER(_RawTable), C.POINTER(_SquigTarget), C.POINTER(_SquigBand),
                                                           C.c_size_t, C.POINTER(_SquigParams), C.c_int, C.c_int, C.POINTER(_SquigResult)]
    L.scrappie_hip_squiggle_diagonal_band.restype = C.c_size_t
    L.scrappie_hip_squiggle_diagonal_band.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, i32p]
    L.scrappie_hip_squiggle_band_lds_max_width.restype = C.c_size_t
    L.scrappie_hip_squiggle_band_lds_max_width.argtypes = []
    L.scrappie_hip_squiggle_band_plan.restype = C.c_longlong
    L.scrappie_hip_squiggle_band_plan.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                                  C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_squiggle_band_form_counts.restype = None
    L.scrappie_hip_squiggle_band_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_squiggle_match_multi_batch.argtypes = [C.c_void_p, C.POINTER(_RawTable), C.POINTER(_SquigCandidates), C.c_size_t,
                                                          C.POINTER(_SquigParams), C.c_int, C.c_int, C.POINTER(_SquigMultiResult)]
    L.scrappie_hip_free_squiggle_multi_results.restype = None
    L.scrappie_hip_free_squiggle_multi_results.argtypes = [C.POINTER(_SquigMultiResult), C.c_size_t]
    L.scrappie_hip_squiggle_match_multi.argtypes = [_RawTable, C.POINTER(_SquigTarget), C.c_size_t, C.POINTER(_SquigParams), C.c_int,
                                                    C.POINTER(C.c_float)]
    L.scrappie_hip_squiggle_pack_plan.restype = C.c_long
    L.scrappie_hip_squiggle_pack_plan.argtypes = [C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    L.scrappie_hip_squiggle_pack_max_cells.restype = C.c_size_t
    L.scrappie_hip_squiggle_pack_max_cells.argtypes = []
    L.scrappie_hip_squiggle_pack_layout.restype = C.c_size_t
    L.scrappie_hip_squiggle_pack_layout.argtypes = [C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.scrappie_hip_squiggle_pack_form_counts.restype = None
    L.scrappie_hip_squiggle_pack_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.squiggle_match_local_viterbi.restype = C.c_float
    L.squiggle_match_local_viterbi.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float, i32p, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    L.squiggle_match_local_forward.restype = C.c_float
    L.squiggle_match_local_forward.argtypes = [_RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float]
    L.scrappie_hip_squiggle_match_local_batch.argtypes = [C.c_void_p, C.POINTER(_RawTable), C.POINTER(_SquigTarget), C.c_size_t,
                                                          C.POINTER(_SquigParams), C.c_int, C.c_int, C.POINTER(_SquigLocalResult)]
    L.scrappie_hip_free_squiggle_local_results.restype = None
    L.scrappie_hip_free_squiggle_local_results.argtypes = [C.POINTER(_SquigLocalResult), C.c_size_t]
    L.scrappie_hip_squiggle_local_plan.restype = C.c_longlong
    L.scrappie_hip_squiggle_local_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_long, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.scrappie_hip_squiggle_local_stride.restype = C.c_size_t
    L.scrappie_hip_squiggle_local_stride.argtypes = [C.c_size_t, C.c_size_t, C.c_long]
    L.scrappie_hip_squiggle_local_max_cells.restype = C.c_size_t
    L.scrappie_hip_squiggle_local_max_cells.argtypes = []
    L.scrappie_hip_squiggle_local_form_counts.restype = None
    L.scrappie_hip_squiggle_local_form_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.scrappie_hip_squiggle_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scrappie_hip_squiggle_lds_max_pos.restype = C.c_size_t
    L.scrappie_hip_map_lds_max_seq.restype = C.c_size_t
    L.scrappie_hip_map_lds_max_seq.argtypes = []
    for nm in ("scrappie_hip_map_plan_scratch", "scrappie_hip_squiggle_plan_scratch"):
        getattr(L, nm).restype = C.c_longlong
        getattr(L, nm).argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_longlong)]
    for nm in ("squiggle_r94", "squiggle_r94_rna", "squiggle_r10"):
        getattr(L, nm).restype = PM
        getattr(L, nm).argtypes = [ip, C.c_size_t, C.c_bool]
    L.scrappie_hip_squiggle_predict_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(ip), sp, C.c_size_t, C.c_int, C.POINTER(PM)]
    L.scrappie_hip_sqnet_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scrappie_hip_sqnet_tile.restype = C.c_size_t
    L.scrappie_hip_sqnet_tile.argtypes = []
    L.scrappie_hip_sqnet_launch_count.restype = C.c_uint64
    L.scrappie_hip_sqnet_launch_count.argtypes = []
    L.scrappie_hip_crf_post_plan.restype = C.c_longlong
    L.scrappie_hip_crf_post_plan.argtypes = [sp, C.c_size_t, C.POINTER(C.c_longlong)]
    L.scrappie_hip_posterior_crf_batch.argtypes = [C.c_void_p, C.POINTER(PM), C.c_size_t, C.POINTER(PM)]
    L.scrappie_hip_basecall_batch_probs.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.c_size_t, C.POINTER(Params), C.POINTER(_Call),
                                                    C.POINTER(PM)]
    L.scrappie_hip_crf_post_timing.restype = None
    L.scrappie_hip_crf_post_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scrappie_hip_crf_post_launch_count.restype = C.c_uint64
    L.scrappie_hip_crf_post_launch_count.argtypes = []
    L.detect_events.restype = _EventTable
    L.detect_events.argtypes = [_RawTable, DetectorParam]
    L.scrappie_hip_detect_events_host.restype = _EventTable
    L.scrappie_hip_detect_events_host.argtypes = [C.POINTER(C.c_float), C.c_size_t, C.POINTER(DetectorParam), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.scrappie_hip_detect_events_batch.argtypes = [C.c_void_p, C.POINTER(_RawTable), C.c_size_t, C.POINTER(DetectorParam), C.POINTER(_EventResult)]
    L.scrappie_hip_free_event_results.restype = None
    L.scrappie_hip_free_event_results.argtypes = [C.POINTER(_EventResult), C.c_size_t]
    L.scrappie_hip_event_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scrappie_hip_event_tile.restype = C.c_size_t
    L.scrappie_hip_event_tile.argtypes = []
    L.scrappie_hip_event_launch_count.restype = C.c_uint64
    L.scrappie_hip_event_launch_count.argtypes = []
    L.scrappie_hip_events_plan_scratch.restype = C.c_longlong
    L.scrappie_hip_events_plan_scratch.argtypes = [C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_longlong)]
    L.scrappie_hip_events_plan_launches.restype = C.c_long
    L.scrappie_hip_events_plan_launches.argtypes = [C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.c_size_t]
    L.homopolymer_dwell_correction.restype = C.c_void_p
    L.homopolymer_dwell_correction.argtypes = [_EventTable, ip, C.c_size_t, C.c_size_t]
    L.dwell_corrected_overlapper.restype = C.c_void_p
    L.dwell_corrected_overlapper.argtypes = [ip, ip, C.c_int, C.c_int, DwellModel]
    L.scrappie_hip_dwell_scale.restype = C.c_float
    L.scrappie_hip_dwell_scale.argtypes = [_EventTable, C.c_size_t]
    L.scrappie_hip_dwell_capacity.restype = C.c_size_t
    L.scrappie_hip_dwell_capacity.argtypes = [C.c_size_t]
    L.scrappie_hip_debug_stitch_dwell.argtypes = [C.c_void_p, ip, ip, sp, C.c_size_t, C.c_int, fp, C.c_int, sp, C.c_void_p, C.c_size_t, ip, ip, ip]
    L.scrappie_hip_basecall_events_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.c_size_t, C.POINTER(DetectorParam),
                                                     C.POINTER(Params), C.c_int, C.POINTER(_Call)]
    L.sh_dwell_stitch.restype = C.c_void_p       # (internal: the engine's host fallback, for the tests through dwell_stitch_host)
    L.sh_dwell_stitch.argtypes = [ip, ip, C.c_int, C.c_int, C.c_int, C.c_float, ip]
    L.scrappie_hip_read_raw.restype = _RawTable
    L.scrappie_hip_read_raw.argtypes = [C.c_char_p, C.c_bool]
    L.scrappie_hip_launch_form_counts.restype = None
    L.scrappie_hip_launch_form_counts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _lib = L
    return L


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def last_error():
    return lib().scrappie_hip_last_error().decode()


def plan_scratch(kind, sizes, counts):
    """The planner's scratch layout of one launch of reads in this order (host arithmetic, no device): kind 'map' with
    sizes = states and counts = blocks per read, 'squig' with positions and samples, or 'map_crf' with bases and blocks.
    Returns (off, total): the float offset of each read's score rows (-1: in LDS) and the floats allocated for all of them."""
    fn = {"map": lib().scrappie_hip_map_plan_scratch, "squig": lib().scrappie_hip_squiggle_plan_scratch,
          "map_crf": lib().scrappie_hip_map_crf_plan_scratch}[kind]
    a = np.ascontiguousarray(sizes, dtype=np.uintp)
    b = np.ascontiguousarray(counts, dtype=np.uintp)
    off = np.zeros(len(a), dtype=np.longlong)
    sp = C.POINTER(C.c_size_t)
    total = fn(a.ctypes.data_as(sp), b.ctypes.data_as(sp), len(a), off.ctypes.data_as(C.POINTER(C.c_longlong)))
    return off, int(total)


def crf_post_plan(nblocks):
    """Where the base probabilities of one launch of reads of `nblocks` blocks lie in its output buffer (host arithmetic, no device;
    scrappie_hip_crf_post_plan): (off, total) -- the float offset of each read's (nblock + 1) x 5 floats and the floats of all of them."""
    a = np.ascontiguousarray(nblocks, dtype=np.uintp)
    off = np.zeros(len(a), dtype=np.longlong)
    total = lib().scrappie_hip_crf_post_plan(a.ctypes.data_as(C.POINTER(C.c_size_t)), len(a), off.ctypes.data_as(C.POINTER(C.c_longlong)))
    return off, int(total)


def launch_form_counts():
    """Launches of each kernel form in this process so far (scrappie_hip_launch_form_counts): {'map': {(viterbi, banded,
    tiled, scratch): n} for the 16 forms of k_map, 'squig': {(viterbi, scratch): n} for the 4 of k_squig}."""
    m, q = (C.c_uint64 * 16)(), (C.c_uint64 * 4)()
    lib().scrappie_hip_launch_form_counts(m, q)
    return dict(map={(bool(k & 8), bool(k & 4), bool(k & 2), bool(k & 1)): int(m[k]) for k in range(16)},
                squig={(bool(k & 2), bool(k & 1)): int(q[k]) for k in range(4)})


def _form_counts(counts, nbit=3):
    """{(a bool per bit, the highest first): n} of a *_form_counts symbol that fills 2 ** nbit counters"""
    q = (C.c_uint64 * (1 << nbit))()
    counts(q)
    return {tuple(bool(k >> b & 1) for b in reversed(range(nbit))): int(q[k]) for k in range(1 << nbit)}


def _local_plan(plan, *sizes_and_stride):
    """A *_local_plan symbol on its leading arguments: the windows counted, then the arrays filled."""
    nw = int(plan(*sizes_and_stride, 0, None, None, None, None, None, None))
    first, ncell, own = (np.zeros(nw, dtype=np.uintp) for _ in range(3))
    home = np.zeros(nw, dtype=np.int32)
    off = np.zeros(nw, dtype=np.longlong)
    tot = C.c_longlong(0)
    sp = C.POINTER(C.c_size_t)
    plan(*sizes_and_stride, nw, first.ctypes.data_as(sp), ncell.ctypes.data_as(sp), own.ctypes.data_as(sp), home.ctypes.data_as(C.POINTER(C.c_int)),
         off.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(tot))
    return dict(first=first, ncell=ncell, own=own, home=home, scr_off=off, scr_floats=int(tot.value))


def _set_default_engine_option(name, value):
    """A debug option of the process-default engine, the one the per-read functions run on (an `Engine` has `debug_option`)."""
    if lib().scrappie_hip_debug_option(None, name.encode(), int(value)) != 0:
        raise RuntimeError("debug_option: " + last_error())


def _pack_plan(plan, lengths, pack_cells):
    """A *_pack_plan symbol (or scrappie_hip_crf_find_plan) on the members' lengths: (pack, cell, npack)."""
    a = np.ascontiguousarray(lengths, dtype=np.uintp)
    pack = np.full(max(len(a), 1), -1, dtype=np.int32)
    cell = np.full(max(len(a), 1), -1, dtype=np.longlong)
    n = plan(a.ctypes.data_as(C.POINTER(C.c_size_t)), len(a), int(pack_cells), pack.ctypes.data_as(C.POINTER(C.c_int)), cell.ctypes.data_as(C.POINTER(C.c_longlong)))
    return pack[:len(a)], cell[:len(a)], int(n)


def map_crf_form_counts():
    """Launches of each k_map_crf form in this process so far (scrappie_hip_map_crf_form_counts):
    {(viterbi, tiled, scratch): n}."""
    return _form_counts(lib().scrappie_hip_map_crf_form_counts)


def map_crf_local_form_counts():
    """Launches of each k_map_crf_local form in this process so far (scrappie_hip_map_crf_local_form_counts):
    {(viterbi, tiled, scratch): n}."""
    return _form_counts(lib().scrappie_hip_map_crf_local_form_counts)


def map_crf_local_max_cells():
    """The most cells a window of k_map_crf_local keeps in LDS; a larger window keeps its rows in device scratch."""
    return int(lib().scrappie_hip_map_crf_local_max_cells())


def map_crf_local_plan(seq_len, nblock, stride=-1):
    """The cut of the seq_len + 1 cells of a sequence into windows for a read of `nblock` blocks (host arithmetic, no device;
    scrappie_hip_map_crf_local_plan).  `stride`: start cells per window, 0: one window, -1: the default.  Returns a dict of
    arrays, one entry per window: first, ncell, own, home (0 LDS, 1 device scratch), scr_off (-1 in LDS), and scr_floats."""
    return _local_plan(lib().scrappie_hip_map_crf_local_plan, seq_len, nblock, int(stride))


def set_map_crf_local_stride(value):
    """The debug option "map_crf_local_stride" of the process-default engine, the one `map_trans_to_reference` runs on: start
    cells per window, 0: one window, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("map_crf_local_stride", value)


def map_local_form_counts():
    """Launches of each k_map_local form in this process so far (scrappie_hip_map_local_form_counts):
    {(viterbi, tiled, scratch): n}."""
    return _form_counts(lib().scrappie_hip_map_local_form_counts)


def map_local_max_cells(nstate):
    """The most cells a window of k_map_local keeps in LDS beside the two columns of a posterior of `nstate` states; a larger
    window keeps its rows in device scratch."""
    return int(lib().scrappie_hip_map_local_max_cells(nstate))


def map_local_plan(seq_len, nblock, nstate, stride=-1):
    """The cut of the `seq_len` positions of a sequence into windows for a read of `nblock` blocks of a posterior of `nstate`
    states (host arithmetic, no device; scrappie_hip_map_local_plan).  `stride`: entry positions per window, 0: one window, -1:
    the default.  Returns a dict of arrays, one entry per window: first, ncell, own, home (0 LDS, 1 device scratch), scr_off (-1
    in LDS), and scr_floats."""
    return _local_plan(lib().scrappie_hip_map_local_plan, seq_len, nblock, nstate, int(stride))


def set_map_local_stride(value):
    """The debug option "map_local_stride" of the process-default engine, the one `map_post_to_reference` runs on: entry
    positions per window, 0: one window, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("map_local_stride", value)


def crf_find_form_counts():
    """Launches of each k_crf_find form in this process so far (scrappie_hip_crf_find_form_counts): {(positions, tiled): n}."""
    return _form_counts(lib().scrappie_hip_crf_find_form_counts, 2)


def crf_find_max_cells():
    """The most cells a pack of k_crf_find holds, the read's five included; a motif of L bases takes L + 4, so the longest
    motif that can be searched has crf_find_max_cells() - 9 bases."""
    return int(lib().scrappie_hip_crf_find_max_cells())


def crf_find_plan(lengths, pack_cells=512):
    """Motifs of `lengths` bases into packs of at most `pack_cells` cells, in input order (host arithmetic, no device;
    scrappie_hip_crf_find_plan).  Returns (npack, pack, cell): per motif its pack and its first cell there, -1 where the motif
    is empty or too long for k_crf_find."""
    pack, cell, npack = _pack_plan(lib().scrappie_hip_crf_find_plan, lengths, pack_cells)
    return npack, pack, cell


def set_crf_find_cells(value):
    """The debug option "crf_find_cells" of the process-default engine, the one `find_in_trans` runs on: cells per pack of
    motifs, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("crf_find_cells", value)


def map_pack_form_counts():
    """Launches of each k_map_pack form in this process so far (scrappie_hip_map_pack_form_counts): {(viterbi, tiled): n}."""
    return _form_counts(lib().scrappie_hip_map_pack_form_counts, 2)


def map_pack_max_cells():
    """The most cells (a candidate of L states takes L + 2) one pack of k_map_pack holds; a longer candidate takes k_map."""
    return int(lib().scrappie_hip_map_pack_max_cells())


def map_pack_plan(seqlens, pack_cells):
    """The packing of candidates of `seqlens` states into packs of at most `pack_cells` cells (host arithmetic, no device;
    scrappie_hip_map_pack_plan): (pack, cell, npack) -- each candidate's pack (-1: too long for any, it takes k_map) and its
    first cell there."""
    return _pack_plan(lib().scrappie_hip_map_pack_plan, seqlens, pack_cells)


def set_map_pack_cells(value):
    """The debug option "map_pack_cells" of the process-default engine, the one `map_post_to_sequences` runs on: cells per pack
    of candidates, 0: every candidate through k_map, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("map_pack_cells", value)


def squiggle_pack_form_counts():
    """Launches of each k_squig_pack form in this process so far (scrappie_hip_squiggle_pack_form_counts): {viterbi: n}."""
    q = (C.c_uint64 * 2)()
    lib().scrappie_hip_squiggle_pack_form_counts(q)
    return {bool(k): int(q[k]) for k in range(2)}


def squiggle_pack_max_cells():
    """The most cells (a candidate squiggle of npos positions takes npos) one pack of k_squig_pack holds; a longer candidate
    takes k_squig."""
    return int(lib().scrappie_hip_squiggle_pack_max_cells())


def squiggle_pack_plan(npos, pack_cells):
    """The packing of candidate squiggles of `npos` positions into packs of at most `pack_cells` cells (host arithmetic, no
    device; scrappie_hip_squiggle_pack_plan): (pack, cell, npack) -- each candidate's pack (-1: too long for any, it takes
    k_squig) and its first cell there."""
    return _pack_plan(lib().scrappie_hip_squiggle_pack_plan, npos, pack_cells)


def squiggle_pack_layout(npos, pack, which):
    """Pack `which` of a `squiggle_pack_plan` as k_squig_pack reads it (scrappie_hip_squiggle_pack_layout): (wa, wb, piece0,
    npiece, pieces) -- the two words of every cell of the pack, and per candidate of the call its first END piece and how
    many it has (-1 for the candidates of other packs)."""
    a = np.ascontiguousarray(npos, dtype=np.uintp)
    pk = np.ascontiguousarray(pack, dtype=np.int32)
    ncell = int(a[pk == which].sum())
    wa = np.zeros(max(ncell, 1), dtype=np.int32)
    wb = np.zeros(max(ncell, 1), dtype=np.int32)
    piece0 = np.full(max(len(a), 1), -1, dtype=np.int32)
    npiece = np.full(max(len(a), 1), -1, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    n = lib().scrappie_hip_squiggle_pack_layout(a.ctypes.data_as(C.POINTER(C.c_size_t)), len(a), pk.ctypes.data_as(ip), int(which),
                                                wa.ctypes.data_as(ip), wb.ctypes.data_as(ip), piece0.ctypes.data_as(ip), npiece.ctypes.data_as(ip))
    return wa[:ncell], wb[:ncell], piece0[:len(a)], npiece[:len(a)], int(n)


def set_squiggle_pack_cells(value):
    """The debug option "squig_pack_cells" of the process-default engine, the one `squiggle_match_many` runs on: cells per
    pack of candidate squiggles, 0: every candidate through k_squig, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("squig_pack_cells", value)


def squiggle_local_form_counts():
    """Launches of each k_squig_local form in this process so far (scrappie_hip_squiggle_local_form_counts):
    {(viterbi, scratch): n}."""
    return _form_counts(lib().scrappie_hip_squiggle_local_form_counts, 2)


def squiggle_local_max_cells():
    """The most cells a window of k_squig_local keeps in LDS (rows, END row and its slice of the tables); a larger window keeps
    its rows in device scratch."""
    return int(lib().scrappie_hip_squiggle_local_max_cells())


def squiggle_local_plan(npos, nsample, stride=-1):
    """The cut of a reference squiggle of `npos` positions into windows for a read of `nsample` samples (host arithmetic, no
    device; scrappie_hip_squiggle_local_plan).  `stride`: entry positions per window, 0: one window, -1: the default.  Returns a
    dict of arrays, one entry per window: first, ncell, own, home (0 LDS, 1 device scratch), scr_off (-1 in LDS), and
    scr_floats."""
    return _local_plan(lib().scrappie_hip_squiggle_local_plan, npos, nsample, int(stride))


def set_squiggle_local_stride(value):
    """The debug option "squig_local_stride" of the process-default engine, the one `squiggle_match_reference` runs on: entry
    positions per window, 0: one window, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("squig_local_stride", value)


def _squig_targets(squiggles):
    """(the ctypes array of scrappie_hip_squiggle_target for a list of (npos, 3) arrays, what keeps its memory alive)"""
    keep = []
    tgs = (_SquigTarget * max(len(squiggles), 1))()
    for i, sq in enumerate(squiggles):
        sq = np.ascontiguousarray(sq, dtype=ftype)
        if sq.ndim != 2 or (sq.shape[0] and sq.shape[1] < 1):
            raise ValueError("a squiggle should be an (npos, 3) array")
        keep.append(sq)
        tgs[i] = _SquigTarget(sq.ctypes.data_as(C.POINTER(C.c_float)) if sq.size else None, sq.shape[0], sq.shape[1])
    return tgs, keep


def squiggle_match_many(rt, squiggles, rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0, min_score=5.0, viterbi=True):
    """The `RawTable` rt as it is (no trimming), over [rt.start, rt.end), against every one of `squiggles` ((npos, 3) arrays
    or ScrappyMatrix) in one pass on the process-default engine (scrappie_hip_squiggle_match_multi): the float32 raw
    squiggle_match_viterbi / _forward scores, NaN where a squiggle cannot be matched."""
    if not isinstance(rt, RawTable):
        raise TypeError('`rt` should be a RawTable.')
    sqs = [s.data(as_numpy=True, sloika=False) if isinstance(s, ScrappyMatrix) else s for s in squiggles]
    tgs, keep = _squig_targets(sqs)
    p = _SquigParams(rate, back_prob, local_pen, skip_pen, min_score)
    score = np.full(len(sqs), np.nan, dtype=np.float32)
    if lib().scrappie_hip_squiggle_match_multi(rt.data(), tgs, len(sqs), C.byref(p), 1 if viterbi else 0,
                                               score.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise RuntimeError("squiggle_match_multi: " + last_error())
    return score


def map_crf_pack_form_counts():
    """Launches of each k_map_crf_pack form in this process so far (scrappie_hip_map_crf_pack_form_counts): {(viterbi, tiled): n}."""
    return _form_counts(lib().scrappie_hip_map_crf_pack_form_counts, 2)


def map_crf_pack_max_cells():
    """The most cells (a candidate of L bases takes L + 1) one pack of k_map_crf_pack holds; a longer candidate takes k_map_crf."""
    return int(lib().scrappie_hip_map_crf_pack_max_cells())


def map_crf_pack_plan(lengths, pack_cells):
    """The packing of candidates of `lengths` bases into packs of at most `pack_cells` cells (host arithmetic, no device;
    scrappie_hip_map_crf_pack_plan): (pack, cell, npack) -- each candidate's pack (-1: too long for any, it takes k_map_crf) and
    its first cell there."""
    return _pack_plan(lib().scrappie_hip_map_crf_pack_plan, lengths, pack_cells)


def set_map_crf_pack_cells(value):
    """The debug option "map_crf_pack_cells" of the process-default engine, the one `map_trans_to_sequences` runs on: cells per
    pack of candidates, 0: every candidate through k_map_crf, -1: the default.  (An `Engine` has `debug_option`.)"""
    _set_default_engine_option("map_crf_pack_cells", value)


def squiggle_band_form_counts():
    """Launches of each k_squig_band form in this process so far (scrappie_hip_squiggle_band_form_counts):
    {(viterbi, scratch): n}."""
    return _form_counts(lib().scrappie_hip_squiggle_band_form_counts, 2)


def plan_squiggle_band(npos, width, nsample, path=True):
    """The banded planner's layout of one launch of banded reads in this order (host arithmetic, no device;
    scrappie_hip_squiggle_band_plan): dict(scr_off, tb_off: per read, -1 for rows in LDS / no traceback; scr_floats,
    tb_words: what the launch allocates; bytes: what the launch is charged)."""
    a, w, b = (np.ascontiguousarray(v, dtype=np.uintp) for v in (npos, width, nsample))
    if not len(a) == len(w) == len(b):
        raise ValueError("one width and one sample count per read")
    scr, tb = np.zeros(len(a) + 1, dtype=np.longlong), np.zeros(len(a) + 1, dtype=np.longlong)
    sp, lp = C.POINTER(C.c_size_t), C.POINTER(C.c_longlong)
    total = lib().scrappie_hip_squiggle_band_plan(a.ctypes.data_as(sp), w.ctypes.data_as(sp), b.ctypes.data_as(sp), len(a), 1 if path else 0,
                                                  scr.ctypes.data_as(lp), tb.ctypes.data_as(lp))
    return dict(scr_off=scr[:-1], tb_off=tb[:-1], scr_floats=int(scr[-1]), tb_words=int(tb[-1]), bytes=int(total))


def squiggle_diagonal_band(nsample, npos, halfwidth):
    """(low, width) of the diagonal band of half-width `halfwidth` positions for `nsample` samples against `npos` positions
    (scrappie_hip_squiggle_diagonal_band): width = min(npos, 2 h + 1), low[t] = clamp(t * npos // nsample - h, 0, npos - width)."""
    if nsample < 0 or npos < 0 or halfwidth < 0:
        raise ValueError("nsample, npos and halfwidth should not be negative")
    low = np.zeros(nsample, dtype=np.int32)
    width = lib().scrappie_hip_squiggle_diagonal_band(nsample, npos, halfwidth, low.ctypes.data_as(C.POINTER(C.c_int32)))
    return low, int(width)


def _squiggle_band(band, nsample, npos):
    """a `band=` argument for one read of `nsample` mapped samples and `npos` positions as (low int32 array or None, width):
    None, an int (diagonal half-width) or a (low, width) pair as given"""
    if band is None:
        return None, 0
    if isinstance(band, (int, np.integer)):
        return squiggle_diagonal_band(nsample, npos, int(band))
    low, width = band
    low = np.ascontiguousarray(low, dtype=np.int32)
    if low.ndim != 1 or len(low) != nsample:
        raise ValueError("a band's low should have one entry per mapped sample (%d)" % nsample)
    if int(width) < 0:
        raise ValueError("a band's width should not be negative")
    return low, int(width)


def _take_string(ptr):
    if not ptr:
        return None
    s = C.string_at(ptr).decode()
    _libc.free(ptr)
    return s


def _raw_tables(signals):
    """The ctypes raw_table array of a batched call and what keeps its memory alive: each signal is a float32 array (its
    whole length the window) or a `RawTable` with its window."""
    keep = [x if isinstance(x, RawTable) else np.ascontiguousarray(x, dtype=ftype) for x in signals]
    rts = (_RawTable * max(len(keep), 1))()
    for i, x in enumerate(keep):
        rts[i] = x.data() if isinstance(x, RawTable) else _RawTable(None, len(x), 0, len(x), x.ctypes.data_as(C.POINTER(C.c_float)))
    return rts, keep


def _paths(rs, length_attr='nblock', more=0):
    """The paths of a batched mapping call's results rs (a list of its ctypes structs), each an array of `length_attr` + more
    ints; None where a result has none.  (One pass over the whole list: a call per read would show in the calls' wall time.)"""
    as_array = np.ctypeslib.as_array
    return [as_array(r.path, shape=(getattr(r, length_attr) + more,)).copy() if r.path else None for r in rs]


def _scores_and_paths(out, n, length_attr, more=0):
    """[(score, path or None)] of a batched mapping call's results"""
    rs = [out[i] for i in range(n)]
    return [(float(r.score), pth) for r, pth in zip(rs, _paths(rs, length_attr, more))]


def _located(out, n, viterbi, length_attr='nblock', more=0):
    """[(score, first, last, path)] of a batched reference-local call's results: first with a path only, and None for all
    three where the score is NaN or the call summed the windows.  (One pass, as _paths.)"""
    rs = [out[i] for i in range(n)]
    res = []
    for r, pth in zip(rs, _paths(rs, length_attr, more)):
        sc = float(r.score)
        if np.isnan(sc) or not viterbi:
            res.append((sc, None, None, None))
        else:
            res.append((sc, int(r.first) if pth is not None else None, int(r.last), pth))
    return res


def _per_read_references(references, n):
    """`references`: one string for all n reads, or one per read.  Returns one per read."""
    if isinstance(references, str):
        return [references] * n
    if len(references) != n:
        raise ValueError("one reference for all signals, or one per signal")
    return references


def _reference_targets(references, kmer_len):
    """The _MapLocalTarget array for one reference string per read, each distinct one encoded once -- one that cannot be
    encoded as an empty sequence, which the library maps to NaN --, and what keeps its memory alive."""
    tgs = (_MapLocalTarget * max(len(references), 1))()
    enc = {}
    for i, sq in enumerate(references):
        if id(sq) not in enc:
            try:
                enc[id(sq)] = np.ascontiguousarray(encode_bases(sq, kmer_len), dtype=np.int32)
            except ValueError:
                enc[id(sq)] = np.zeros(0, dtype=np.int32)
        codes = enc[id(sq)]
        tgs[i].seq = codes.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(codes)
    return tgs, enc


def _path_needs_viterbi(path, viterbi):
    if path and not viterbi:
        raise ValueError('Cannot calulate path with `viterbi==False`.')


def _per_read_lists(lists, n, what):
    """`lists`: one list of strings shared by all n reads, or one list of strings per read.  Returns (the lists, shared)."""
    lists = list(lists)
    shared = all(isinstance(c, str) for c in lists)
    if not shared:
        if any(isinstance(c, str) for c in lists):
            raise ValueError("`%s`: a list of strings for every read, or one list of strings per read" % what)
        if len(lists) != n:
            raise ValueError("one list of %s per signal" % what)
    return lists, shared


def _per_read_sets(lists, shared, n, targets):
    """The scrappie_hip_map_candidates array of n reads for what _per_read_lists returned, and what keeps its memory alive;
    targets(list) makes (the ctypes target array, what keeps it alive) -- once for a shared list."""
    cds = (_MapCandidates * max(n, 1))()
    if shared:
        made = [targets(lists)]
        tgs, k = made[0][0], len(lists)
        for i in range(n):
            cds[i].cand, cds[i].ncand = tgs, k
    else:
        made = []
        for i, c in enumerate(lists):
            c = list(c)
            made.append(targets(c))
            cds[i].cand, cds[i].ncand = made[i][0], len(c)
    return cds, made


# ---------------------------------------------------------------------------
# scrappy-compatible objects (python/scrappy/__init__.py:47-273)
# ---------------------------------------------------------------------------
class RawTable(object):
    """Representation of a scrappie `raw_table` (python/scrappy/__init__.py:47-112)."""

    def __init__(self, data, start=0, end=None):
        if end is None:
            end = len(data)
        self._data = np.ascontiguousarray(np.asarray(data).astype(ftype, order='C', copy=True))
        self._rt = _RawTable(None, len(self._data), start, end,
                             self._data.ctypes.data_as(C.POINTER(C.c_float)))

    def data(self, as_numpy=False):
        if as_numpy:
            return np.copy(self._data[self.start:self.end])
        return self._rt

    @property
    def start(self):
        return self._rt.start

    @property
    def end(self):
        return self._rt.end

    def trim(self, start=200, end=10, varseg_chunk=100, varseg_thresh=0.0):
        """python/scrappy/__init__.py:92-133 (== trim_and_segment_raw, scrappie_common.c:11-17,
        except that the data array is kept when the window comes out empty)."""
        rt = lib().trim_raw_by_mad(self._rt, varseg_chunk, varseg_thresh)
        rt.start = rt.start + start if (rt.n - rt.start) > start else rt.n
        rt.end = rt.end - end if rt.end > end else 0
        if rt.start >= rt.end:
            rt.start, rt.end = 0, 0
        self._rt = rt
        return self

    def scale(self):
        """python/scrappy/__init__.py:107-112, :136-147"""
        n = self._rt.end - self._rt.start
        if n > 0:
            ptr = C.cast(C.addressof(self._rt.raw.contents) + 4 * self._rt.start, C.POINTER(C.c_float))
            lib().medmad_normalise_array(ptr, n)
        return self


class ScrappyMatrix(object):
    """Owns a `scrappie_matrix` returned by the library (python/scrappy/__init__.py:150-200)."""

    def __init__(self, scrappy_matrix):
        self._data = scrappy_matrix
        self.shape = (self._data.contents.nc, self._data.contents.nr)

    def __del__(self):
        if getattr(self, "_data", None):
            lib().free_scrappie_matrix(self._data)
            self._data = None

    def data(self, as_numpy=False, sloika=True):
        if as_numpy:
            return _scrappie_to_numpy(self._data, sloika=sloika)
        return self._data

    @classmethod
    def from_numpy(cls, array, sloika=True):
        """array is (blocks, states); with sloika=True the stay state is first."""
        a = np.asarray(array, dtype=ftype)
        if sloika:
            a = np.hstack((a[:, 1:], a[:, 0:1]))
        a = np.ascontiguousarray(a)
        m = lib().mat_from_array(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0])
        return cls(m)


def _scrappie_to_numpy(matrix, sloika=True):
    """python/scrappy/__init__.py:247-273: drop the SSE padding; optionally roll
    the stay state to the front (sloika order)."""
    m = matrix.contents
    flat = np.ctypeslib.as_array(C.cast(m.data, C.POINTER(C.c_float)), shape=(m.nc * vsize * m.nrq,))
    np_matrix = flat.reshape(m.nc, vsize * m.nrq)[:, :m.nr]
    if sloika:
        np_matrix = np.hstack((np_matrix[:, m.nr - 1:m.nr], np_matrix[:, 0:m.nr - 1]))
    return np.array(np_matrix, dtype=ftype, order='C', copy=True)   # a copy: the matrix may be freed


_model_fn_ = {
    'raw_r94': 'nanonet_raw_posterior',
    'rgrgr_r94': 'nanonet_rgrgr_r94_posterior',
    'rgrgr_r941': 'nanonet_rgrgr_r941_posterior',
    'rgrgr_r10': 'nanonet_rgrgr_r10_posterior',
    'rnnrf_r94': 'nanonet_rnnrf_r94_transitions',
}


def _take_events(et):
    """the structured array (synth.EVENT_DTYPE) of an event_table the library malloc'd, which is freed; None for no table"""
    if not et.event:
        return None
    from .synth import EVENT_DTYPE
    ev = np.frombuffer(C.string_at(et.event, et.n * C.sizeof(_Event)), dtype=EVENT_DTYPE).copy()
    _libc.free(C.cast(et.event, C.c_void_p))
    return ev[et.start:et.end]


def detect_events(signal, window_length1=3, window_length2=6, threshold1=1.4, threshold2=9.0, peak_height=0.2):
    """The reference's detect_events (event_detection.c:268) on a signal in pA (a float32 array, or a `RawTable` with its
    window), on the process-default engine: a structured array with the event_t layout (scrappie_amd.synth.EVENT_DTYPE;
    pos = state = -1), or None where the read has no peak (the reference is undefined there; `last_error()` says so)."""
    rts, keep = _raw_tables([signal])
    return _take_events(lib().detect_events(rts[0], DetectorParam(window_length1, window_length2, threshold1, threshold2, peak_height)))


def detect_events_host(signal, tstats=False, **params):
    """The host statement of detect_events (what the kernels are held against): the event table or None; with `tstats`
    also the two t-statistics."""
    x = np.ascontiguousarray(signal, dtype=ftype)
    fp = C.POINTER(C.c_float)
    t1, t2 = np.zeros(len(x), dtype=ftype), np.zeros(len(x), dtype=ftype)
    p = DetectorParam(**params)
    ev = _take_events(lib().scrappie_hip_detect_events_host(x.ctypes.data_as(fp), len(x), C.byref(p), t1.ctypes.data_as(fp), t2.ctypes.data_as(fp)))
    return (ev, t1, t2) if tstats else ev


def plan_event_scratch(nsample):
    """(off, total): the first scratch slot of each read of one event-detection launch of reads in this order, and the
    slots of the launch (host arithmetic; read i owns nsample[i] + 1 slots of 28 bytes)"""
    a = np.ascontiguousarray(nsample, dtype=np.uintp)
    off = np.zeros(len(a), dtype=np.longlong)
    total = lib().scrappie_hip_events_plan_scratch(a.ctypes.data_as(C.POINTER(C.c_size_t)), len(a), off.ctypes.data_as(C.POINTER(C.c_longlong)))
    return off, int(total)


def plan_event_launches(nsample, budget_slots):
    """(order, starts): the reads of an event-detection call sorted by length, longest first, and the first position in
    that order of each launch under a budget of sample slots; None where one read alone exceeds the budget"""
    a = np.ascontiguousarray(nsample, dtype=np.uintp)
    order = np.zeros(len(a), dtype=np.uint32)
    starts = np.zeros(max(len(a), 1), dtype=np.uintp)
    ng = lib().scrappie_hip_events_plan_launches(a.ctypes.data_as(C.POINTER(C.c_size_t)), len(a), budget_slots,
                                                 order.ctypes.data_as(C.POINTER(C.c_uint32)), starts.ctypes.data_as(C.POINTER(C.c_size_t)), len(starts))
    return None if ng < 0 else (order, starts[:ng].astype(np.int64))


def event_features(events, start=0, end=None):
    """Windowed, studentised features of an event table (networks.c:155-157) as an
    (nevent, 12) float32 array -- the input of an events model.  `events`: structured array
    with the reference's event_t layout (scrappie_amd.synth.EVENT_DTYPE)."""
    ev = np.ascontiguousarray(events)
    if ev.dtype.itemsize != C.sizeof(_Event):
        raise ValueError("events must have the event_t layout (%d bytes per event)" % C.sizeof(_Event))
    end = len(ev) if end is None else end
    et = _EventTable(len(ev), start, end, C.cast(ev.ctypes.data, C.POINTER(_Event)))
    out = np.zeros((end - start, 12), dtype=ftype)
    L = lib()
    L.scrappie_hip_event_features.restype = C.c_int
    L.scrappie_hip_event_features.argtypes = [_EventTable, C.POINTER(C.c_float)]
    if L.scrappie_hip_event_features(et, out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise RuntimeError("event_features failed")
    return out


def _event_table(events):
    """the ctypes event_table over a structured array with the event_t layout, and the array that keeps its memory alive"""
    ev = np.ascontiguousarray(events)
    if ev.dtype.itemsize != C.sizeof(_Event):
        raise ValueError("events must have the event_t layout (%d bytes per event)" % C.sizeof(_Event))
    return _EventTable(len(ev), 0, len(ev), C.cast(ev.ctypes.data, C.POINTER(_Event))), ev


def dwell_corrected_overlapper(path, dwell, nkmer, scale, base_adj=(0.0, 0.0, 0.0, 0.0)):
    """decode.c:516: the k-mer stitching of `path` with every homopolymer entered behind the first k-mer given
    round(its dwell / scale) bases; `dwell`: an int per path entry.  The string as strlen sees the reference's (a call
    that ends inside a homopolymer is one base short of its length); None where the path has no k-mer."""
    path = np.ascontiguousarray(path, dtype=np.int32)
    dwell = np.ascontiguousarray(dwell, dtype=np.int32)
    if len(path) != len(dwell):
        raise ValueError("a dwell per path entry")
    ip = C.POINTER(C.c_int)
    dm = DwellModel(scale, (C.c_float * 4)(*base_adj))
    return _take_string(lib().dwell_corrected_overlapper(path.ctypes.data_as(ip), dwell.ctypes.data_as(ip), len(path), nkmer, dm))


def homopolymer_dwell_correction(events, path, nstate, basecall_len):
    """decode.c:645: the dwell-corrected call of a read from its events -- annotated with `pos` (overlapper's) and
    `state` (1 + path), as scrappie_events.c:308-311 leaves them -- its path (an entry per event) and the length of
    its plain call.  None where the path has no k-mer."""
    et, keep = _event_table(events)
    path = np.ascontiguousarray(path, dtype=np.int32)
    if len(path) < len(keep):
        raise ValueError("a path entry per event")
    return _take_string(lib().homopolymer_dwell_correction(et, path.ctypes.data_as(C.POINTER(C.c_int)), nstate, basecall_len))


def dwell_scale(events, basecall_len):
    """the homo_scale homopolymer_dwell_correction divides the dwells by (decode.c:666-693), a float32"""
    et, keep = _event_table(events)
    return np.float32(lib().scrappie_hip_dwell_scale(et, basecall_len))


def dwell_stitch_host(path, dwell, nstate, prior_num):
    """What the engine's host fallback makes of a read it holds as arrays (sh_host.c: sh_dwell_stitch): `path` has len(dwell)
    entries, or one more (the decoder's last, without an event); returns (bases or None, overlapper's pos[])."""
    path = np.ascontiguousarray(path, dtype=np.int32)
    dwell = np.ascontiguousarray(dwell, dtype=np.int32)
    if len(path) - len(dwell) not in (0, 1):
        raise ValueError("a path of len(dwell) entries, or one more")
    ip = C.POINTER(C.c_int)
    pos = np.zeros(len(path), np.int32)
    s = lib().sh_dwell_stitch(path.ctypes.data_as(ip), dwell.ctypes.data_as(ip), len(dwell), len(path) - len(dwell), nstate, float(prior_num),
                              pos.ctypes.data_as(ip))
    return _take_string(s), pos


def read_raw(path, scale_to_pA=True):
    """A read's samples from a fast5 file (or a headerless .f32 / .i16 file) as (float32 array, uuid or ''); None where it cannot be read."""
    rt = lib().scrappie_hip_read_raw(os.fsencode(path), scale_to_pA)
    if not rt.raw:
        return None
    x = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
    _libc.free(C.cast(rt.raw, C.c_void_p))
    return x, (rt.uuid or b"").decode()


def dwell_capacity(nentry):
    """bytes of bases the engine reserves for a read of `nentry` path entries when the dwell correction is on"""
    return int(lib().scrappie_hip_dwell_capacity(nentry))


def register_model(name, path):
    """Bind a `.scrm` weight container to a reference model name for the per-read
    surface (the reference compiles its weights in; here they are data)."""
    if lib().scrappie_hip_register_model(name.encode(), os.fsencode(path)) < 0:
        raise RuntimeError(last_error())


def calc_post(rt, model='rgrgr_r94', min_prob=1e-6, log=True, tempW=1.0, tempb=1.0):
    """python/scrappy/__init__.py:276-299"""
    if not log and model == 'rnnrf_r94':
        raise ValueError("Returning non-log transformed matrix not supported for model type 'rnnrf_r94'.")
    if not isinstance(rt, RawTable):
        raise TypeError('`rt` should be a RawTable.')
    try:
        fn = getattr(lib(), _model_fn_[model])
    except KeyError:
        raise KeyError("Model type '{}' not recognised.".format(model))
    matrix = fn(rt.data(), min_prob, tempW, tempb, log)
    if not matrix:
        raise RuntimeError('An unknown error occurred during posterior calculation: ' + last_error())
    return ScrappyMatrix(matrix)


def _decode_post(post, stay_pen=0.0, skip_pen=0.0, local_pen=2.0, use_slip=False):
    """python/scrappy/__init__.py:323-346"""
    nblock, nstate = post.shape
    path = np.zeros(nblock + 1, dtype=np.int32)
    score = lib().decode_transducer(post.data(), stay_pen, skip_pen, local_pen,
                                    path.ctypes.data_as(C.POINTER(C.c_int)), use_slip)
    pos = np.zeros(nblock + 1, dtype=np.int32)
    basecall = lib().overlapper(path.ctypes.data_as(C.POINTER(C.c_int)), nblock + 1, nstate - 1,
                                pos.ctypes.data_as(C.POINTER(C.c_int)))
    return _take_string(basecall), score, pos


def _decode_post_crf(post):
    """python/scrappy/__init__.py:349-365"""
    nblock, nstate = post.shape
    path = np.zeros(nblock + 1, dtype=np.int32)
    score = lib().decode_crf(post.data(), path.ctypes.data_as(C.POINTER(C.c_int)))
    pos = np.zeros(nblock + 1, dtype=np.int32)
    basecall = lib().crfpath_to_basecall(path.ctypes.data_as(C.POINTER(C.c_int)), nblock,
                                         pos.ctypes.data_as(C.POINTER(C.c_int)))
    return _take_string(basecall), score, pos


_decoders_ = {'raw_r94': _decode_post, 'rgrgr_r94': _decode_post, 'rgrgr_r941': _decode_post, 'rgrgr_r10': _decode_post,
              'rnnrf_r94': _decode_post_crf}


def decode_post(post, model='rgrgr_r94', **kwargs):
    """python/scrappy/__init__.py:302-320"""
    if not isinstance(post, ScrappyMatrix):
        raise TypeError('`post` should be a ScrappyMatrix.')
    try:
        decoder = _decoders_[model]
    except KeyError:
        raise KeyError("Model type '{}' not recognised.".format(model))
    return decoder(post, **kwargs)


def get_model_stride(model):
    """python/scrappy/__init__.py:389-400"""
    stride = lib().get_raw_model_stride_from_string(model.encode())
    if stride == -1:
        raise ValueError("Invalid scrappie model '{}'.".format(model))
    return stride


def basecall_raw(data, model='rgrgr_r94', with_base_probs=False, **kwargs):
    """python/scrappy/__init__.py:403-430: trim -> scale -> posterior (min_prob
    1e-6) -> decode; no homopolymer correction on this path (quirk Q10)."""
    raw = RawTable(data)
    raw.trim().scale()
    post = calc_post(raw, model, log=True)
    seq, score, pos = decode_post(post, model, **kwargs)
    base_probs = None
    if with_base_probs:
        bp = lib().posterior_crf(post.data())
        base_probs = _scrappie_to_numpy(bp, sloika=False)
        lib().free_scrappie_matrix(bp)
    return seq, score, pos, raw.start, raw.end, base_probs


# ---------------------------------------------------------------------------
# batched engine (additive; the fast path)
# ---------------------------------------------------------------------------
def _gsp():
    """python/scrappy/__init__.py:25-44: alphabet size and k-mer length from a transducer's state count"""
    import itertools
    pairs = [(a, k) for a, k in itertools.product(range(4, 8), range(1, 10))]
    lookup = {a ** k: (a, k) for a, k in pairs}
    assert len(lookup) == len(pairs)

    def guess_state_properties(nstate):
        return lookup[nstate - 1]
    return guess_state_properties


guess_state_properties = _gsp()


def encode_bases(sequence, kmer_len):
    """encode_bases_to_integers: the state codes of `sequence`'s k-mers as an int32 array (ValueError on a base outside ACGT)."""
    b = sequence.encode()
    n = len(b) - kmer_len + 1
    ptr = lib().encode_bases_to_integers(b, len(b), kmer_len)
    if not ptr:
        raise ValueError("cannot encode sequence: " + last_error())
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int)), shape=(n,)).copy()
    _libc.free(ptr)
    return out


def diagonal_bands(bands, nblock, seq_len):
    """python/scrappy/__init__.py:550-558: the (low, high) uintp arrays of a diagonal band of half-width `bands` * seq_len / nblock."""
    gradient = seq_len / nblock
    bands = 2 * bands * gradient
    hband = bands / 2
    return [np.ascontiguousarray(np.array(x, dtype=np.uintp)) for x in (
        [(max(0, x * gradient - hband)) for x in range(nblock)],
        [(min(seq_len, x * gradient + hband)) for x in range(nblock)])]


def map_post_to_sequence(post, sequence, stay_pen=0, skip_pen=0, local_pen=4.0, viterbi=False, path=False, bands=None):
    """python/scrappy/__init__.py:492-578: block-based local-global alignment of a posterior (a `ScrappyMatrix` of
    log-probabilities, as from `calc_post`) to a base sequence, Viterbi or forward, full or banded; the DP runs on the
    GPU.  `bands`: None, an int (diagonal band) or a (low, high) pair.  Returns (score, path or None)."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(post, ScrappyMatrix):
        raise TypeError('`post` should be a ScrappyMatrix.')
    nblock, nstate = post.shape
    alpha_len, kmer_len = guess_state_properties(nstate)
    seq_len = len(sequence) - kmer_len + 1
    ptr = lib().encode_bases_to_integers(sequence.encode(), len(sequence), kmer_len)
    if not ptr:
        raise RuntimeError('An unknown error occurred whilst encoding sequence.')
    try:
        p_seq = C.cast(ptr, C.POINTER(C.c_int))
        path_data = np.zeros(nblock, dtype=np.int32) if (viterbi and path) else None
        p_path = path_data.ctypes.data_as(C.POINTER(C.c_int)) if path_data is not None else None
        if bands is None:
            if viterbi:
                score = lib().map_to_sequence_viterbi(post.data(), stay_pen, skip_pen, local_pen, p_seq, seq_len, p_path)
            else:
                score = lib().map_to_sequence_forward(post.data(), stay_pen, skip_pen, local_pen, p_seq, seq_len)
        else:
            if isinstance(bands, int):
                bands = diagonal_bands(bands, nblock, seq_len)
            elif len(bands) == 2:
                bands = [np.ascontiguousarray(x, dtype=np.uintp) for x in bands]
            else:
                raise ValueError('`bands` should be `None`, an integer, or length 2.')
            p_lo, p_hi = (x.ctypes.data_as(C.POINTER(C.c_size_t)) for x in bands)
            if not lib().are_bounds_sane(p_lo, p_hi, nblock, seq_len):
                raise ValueError('Supplied banding structure is not valid.')
            func = lib().map_to_sequence_viterbi_banded if viterbi else lib().map_to_sequence_forward_banded
            score = func(post.data(), stay_pen, skip_pen, local_pen, p_seq, seq_len, p_lo, p_hi)
    finally:
        _libc.free(ptr)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score, path_data


def _map_targets(sequences, kmer_len):
    """The ctypes scrappie_hip_map_target array of `sequences` (unbanded) and what keeps its memory alive; a sequence that
    cannot be encoded becomes an empty one, which the library answers with NaN."""
    tgs = (_MapTarget * max(len(sequences), 1))()
    keep = []
    for i, sq in enumerate(sequences):
        try:
            codes = encode_bases(sq, kmer_len)
        except ValueError:
            codes = np.zeros(0, dtype=np.int32)
        keep.append(codes)
        tgs[i].seq = codes.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(codes)
    return tgs, keep


def map_post_to_sequences(post, sequences, stay_pen=0, skip_pen=0, local_pen=4.0, viterbi=False):
    """`map_post_to_sequence`'s score of a posterior (a `ScrappyMatrix` of log-probabilities) against each of `sequences`, in one
    pass on the GPU: the candidates are packed into workgroups of k_map_pack (scrappie_hip_map_post_multi).  Returns a float32
    array of raw scores, one per sequence, NaN where a sequence cannot be mapped; sequences of different lengths are compared as
    they are."""
    if not isinstance(post, ScrappyMatrix):
        raise TypeError('`post` should be a ScrappyMatrix.')
    nblock, nstate = post.shape
    kmer_len = guess_state_properties(nstate)[1]
    tgs, keep = _map_targets(sequences, kmer_len)
    score = np.full(len(sequences), np.nan, dtype=np.float32)
    if lib().scrappie_hip_map_post_multi(post.data(), stay_pen, skip_pen, local_pen, tgs, len(sequences), 1 if viterbi else 0,
                                         score.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score


def map_crf_diagonal_band(nblock, seq_len, halfwidth):
    """(low, high) uintp arrays, nblock + 1 entries each: the diagonal band of half-width `halfwidth` cells of a read of `nblock`
    blocks of a flip-flop (CRF) model against `seq_len` bases (scrappie_hip_map_crf_diagonal_band); always a valid band."""
    lo, hi = np.zeros(nblock + 1, dtype=np.uintp), np.zeros(nblock + 1, dtype=np.uintp)
    sp = C.POINTER(C.c_size_t)
    if lib().scrappie_hip_map_crf_diagonal_band(nblock, seq_len, halfwidth, lo.ctypes.data_as(sp), hi.ctypes.data_as(sp)) != 0:
        raise ValueError("a diagonal band needs at least one block and one base")
    return [lo, hi]


def map_crf_path_band(path, seq_len, halfwidth):
    """(low, high) uintp arrays, nblock + 1 entries each: the band of half-width `halfwidth` cells around a Viterbi path of a
    flip-flop (CRF) model, as `map_trans_to_sequence(..., viterbi=True, path=True)` and `Engine.map_to_sequence(..., path=True)`
    return it (path[t]: the index of the last base emitted through entry t, -1 while none) against `seq_len` bases
    (scrappie_hip_map_crf_path_band): low = max(path + 1 - halfwidth, 0), low[0] = 0, high = min(path + 2 + halfwidth,
    seq_len + 1); always a valid band that holds the path.  ValueError where `path` is no path of such a sequence."""
    p = np.ascontiguousarray(path, dtype=np.int32)
    if p.ndim != 1 or len(p) < 2 or halfwidth < 0:
        raise ValueError("a path has nblock + 1 >= 2 entries, and a half-width is not negative")
    lo, hi = np.zeros(len(p), dtype=np.uintp), np.zeros(len(p), dtype=np.uintp)
    sp = C.POINTER(C.c_size_t)
    if lib().scrappie_hip_map_crf_path_band(p.ctypes.data_as(C.POINTER(C.c_int)), len(p) - 1, seq_len, int(halfwidth), lo.ctypes.data_as(sp),
                                            hi.ctypes.data_as(sp)) != 0:
        raise ValueError("not a path of a sequence of %d bases: entries -1 .. %d, steps of 0 or 1, the last entry %d" % (seq_len, seq_len - 1, seq_len - 1))
    return [lo, hi]


def map_path_band(path, nstate, halfwidth):
    """(low, high) uintp arrays, nblock entries each: the band of half-width `halfwidth` >= 1 states around a Viterbi path of a
    transducer model, as `map_post_to_sequence(..., viterbi=True, path=True)` and `Engine.map_to_sequence(..., path=True)` return
    it (path[t]: the state after block t, -1 in START and END) against `nstate` = len(seq) - k + 1 k-mer states
    (scrappie_hip_map_path_band): with p the position -- 0 over the leading -1s, nstate - 1 over the trailing ones --
    low = max(p - halfwidth, 0), high = min(p + halfwidth + 1, nstate), low[0] = 0, high[-1] = nstate; always a band that
    `are_bounds_sane` accepts and that holds the path.  ValueError where `path` is no path of such a sequence or halfwidth < 1."""
    p = np.ascontiguousarray(path, dtype=np.int32)
    if p.ndim != 1 or len(p) < 1 or halfwidth < 1 or nstate < 1:
        raise ValueError("a path has nblock >= 1 entries, a sequence at least one state, and a half-width is at least 1")
    lo, hi = np.zeros(len(p), dtype=np.uintp), np.zeros(len(p), dtype=np.uintp)
    sp = C.POINTER(C.c_size_t)
    if lib().scrappie_hip_map_path_band(p.ctypes.data_as(C.POINTER(C.c_int)), len(p), int(nstate), int(halfwidth), lo.ctypes.data_as(sp),
                                        hi.ctypes.data_as(sp)) != 0:
        raise ValueError("not a path of a sequence of %d states: -1s, then 0 .. %d in steps of 0, 1 or 2, then -1s" % (nstate, nstate - 1))
    return [lo, hi]


def _map_band(bands, nblock, nstate):
    """`bands` of one transducer read as a (low, high) pair of contiguous uintp arrays: an int is scrappy's `diagonal_bands`"""
    if isinstance(bands, (int, np.integer)):
        return diagonal_bands(int(bands), nblock, nstate)
    if len(bands) != 2:
        raise ValueError('`bands` should be `None`, an integer, or length 2.')
    return [np.ascontiguousarray(x, dtype=np.uintp) for x in bands]


def _crf_band(bands, nblock, seq_len):
    """`bands` of one read as a (low, high) pair of contiguous uintp arrays: an int is the half-width of the diagonal band"""
    if isinstance(bands, (int, np.integer)):
        return map_crf_diagonal_band(nblock, seq_len, int(bands))
    if len(bands) != 2:
        raise ValueError('`bands` should be `None`, an integer, or length 2.')
    return [np.ascontiguousarray(x, dtype=np.uintp) for x in bands]


def map_trans_to_sequence(trans, sequence, viterbi=False, path=False, bands=None):
    """Global alignment of a read's transitions under a flip-flop (CRF) model (a `ScrappyMatrix` of 25 rows, as
    `calc_post(rt, model='rnnrf_r94')` gives) to a base sequence: decode_crf's recursion restricted to the paths that spell the
    sequence, Viterbi or forward, full or banded; the DP runs on the GPU (k_map_crf).  `bands`: None, an int (half-width in
    cells of the diagonal band) or a (low, high) pair of nblock + 1 entries each: the cells -- bases emitted so far, 0 .. len --
    an entry of the path may be in.  Returns (score, path or None); path[t], t = 0 .. nblock, is the index of the last base
    emitted through entry t, -1 while none."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(trans, ScrappyMatrix):
        raise TypeError('`trans` should be a ScrappyMatrix.')
    nblock, nstate = trans.shape
    if nstate != 25:
        raise ValueError('`trans` should hold the 25 transitions of a flip-flop (CRF) model per block.')
    codes = encode_bases(sequence, 1).astype(np.int32)
    seq_len = len(codes)
    p_seq = codes.ctypes.data_as(C.POINTER(C.c_int))
    path_data = np.zeros(nblock + 1, dtype=np.int32) if (viterbi and path) else None
    p_path = path_data.ctypes.data_as(C.POINTER(C.c_int)) if path_data is not None else None
    if bands is None:
        if viterbi:
            score = lib().map_crf_to_sequence_viterbi(trans.data(), p_seq, seq_len, p_path)
        else:
            score = lib().map_crf_to_sequence_forward(trans.data(), p_seq, seq_len)
    else:
        if isinstance(bands, (int, np.integer)):
            bands = map_crf_diagonal_band(nblock, seq_len, int(bands))
        elif len(bands) == 2:
            bands = [np.ascontiguousarray(x, dtype=np.uintp) for x in bands]
        else:
            raise ValueError('`bands` should be `None`, an integer, or length 2.')
        if len(bands[0]) != nblock + 1 or len(bands[1]) != nblock + 1:
            raise ValueError('Supplied banding structure is not valid: nblock + 1 entries each.')
        p_lo, p_hi = (x.ctypes.data_as(C.POINTER(C.c_size_t)) for x in bands)
        if not lib().scrappie_hip_map_crf_bounds_sane(p_lo, p_hi, nblock, seq_len):
            raise ValueError('Supplied banding structure is not valid.')
        if viterbi:
            score = lib().map_crf_to_sequence_viterbi_banded(trans.data(), p_seq, seq_len, p_lo, p_hi, p_path)
        else:
            score = lib().map_crf_to_sequence_forward_banded(trans.data(), p_seq, seq_len, p_lo, p_hi)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score, path_data


def _crf_targets(sequences):
    """The ctypes scrappie_hip_map_target array of `sequences` (base strings, or arrays of base codes, which the library checks)
    and what keeps its memory alive; a string that cannot be encoded becomes an empty sequence, which the library answers with
    NaN."""
    tgs = (_MapTarget * max(len(sequences), 1))()
    keep = []
    for i, sq in enumerate(sequences):
        if isinstance(sq, str):
            try:
                codes = np.ascontiguousarray(encode_bases(sq, 1), dtype=np.int32) if len(sq) else np.zeros(0, dtype=np.int32)
            except ValueError:
                codes = np.zeros(0, dtype=np.int32)
        else:
            codes = np.ascontiguousarray(sq, dtype=np.int32)
        keep.append(codes)
        tgs[i].seq = codes.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(codes)
    return tgs, keep


def map_trans_to_sequences(trans, sequences, viterbi=False):
    """`map_trans_to_sequence`'s score of a read's transitions under a flip-flop (CRF) model (a `ScrappyMatrix` of 25 rows)
    against each of `sequences` (base strings, or arrays of base codes 0..3), unbanded, in one pass on the GPU: the candidates
    are packed into workgroups of k_map_crf_pack (scrappie_hip_map_trans_multi).  Returns a float32 array of scores, one per
    sequence, bit for bit what `map_trans_to_sequence` gives for it; NaN where a sequence cannot be mapped (empty, not bases,
    more bases than the read has entries: `last_error()` names the first)."""
    if not isinstance(trans, ScrappyMatrix):
        raise TypeError('`trans` should be a ScrappyMatrix.')
    nblock, nstate = trans.shape
    if nstate != 25:
        raise ValueError('`trans` should hold the 25 transitions of a flip-flop (CRF) model per block.')
    sequences = list(sequences)
    tgs, keep = _crf_targets(sequences)
    score = np.full(len(sequences), np.nan, dtype=np.float32)
    if lib().scrappie_hip_map_trans_multi(trans.data(), tgs, len(sequences), 1 if viterbi else 0,
                                          score.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score


def apply_edit(seq, kind, i, c=None):
    """The sequence a single-base edit makes of `seq` (a base string, or an array of base codes 0..3): kind 'sub' puts `c` at
    position i < L, 'del' removes position i < L, 'ins' puts `c` before position i <= L.  `c`: a base code 0..3 or one of
    'ACGT'.  Returns what it was given, a string or an int32 array: how `map_trans_edits` and `Engine.score_edits` number their
    results -- sub[i][c], dele[i], ins[i][c] score apply_edit(seq, 'sub' / 'del' / 'ins', i, c)."""
    text = isinstance(seq, str)
    codes = list(seq) if text else [int(b) for b in seq]
    L = len(codes)
    if kind not in ('sub', 'del', 'ins'):
        raise ValueError("`kind` is one of 'sub', 'del', 'ins'")
    if not 0 <= i < L + (1 if kind == 'ins' else 0):
        raise ValueError("position %d is outside a sequence of %d bases for '%s'" % (i, L, kind))
    if kind != 'del':
        if isinstance(c, str):
            if len(c) != 1 or c not in 'ACGT':
                raise ValueError("`c` is one of 'ACGT' or a code 0..3")
            c = c if text else 'ACGT'.index(c)
        elif c is None or not 0 <= int(c) <= 3:
            raise ValueError("`c` is one of 'ACGT' or a code 0..3")
        else:
            c = 'ACGT'[int(c)] if text else int(c)
    out = codes[:i] + ([] if kind == 'del' else [c]) + codes[i + (0 if kind == 'ins' else 1):]
    return ''.join(out) if text else np.array(out, dtype=np.int32)


def _edits_forms(fn, ctype=C.c_uint64, widths=(None,)):
    """a table of the ABI over the forms of the edit kernels (counts, or scratch bytes) as a dict: eight rows forms, then four combining
    forms per width of `widths` (None: the one width, which the key leaves out)"""
    q = (ctype * (8 + 4 * len(widths)))()
    fn(q)
    out = {('rows', bool(k & 4), bool(k & 2), bool(k & 1)): int(q[k]) for k in range(8)}
    for j, w in enumerate(widths):
        out.update({('edits', bool(k & 2), bool(k & 1)) + (() if w is None else (w,)): int(q[8 + 4 * j + k]) for k in range(4)})
    return out


def crf_edits_form_counts():
    """Launches of each form of the edit kernels in this process so far (scrappie_hip_crf_edits_form_counts):
    {('rows', viterbi, tiled, backward): n, ('edits', viterbi, tiled): n}."""
    return _edits_forms(lib().scrappie_hip_crf_edits_form_counts)


def crf_edits_band_form_counts():
    """The same for the banded forms of the edit kernels (scrappie_hip_crf_edits_band_form_counts); `crf_edits_form_counts`
    counts the unbanded forms alone."""
    return _edits_forms(lib().scrappie_hip_crf_edits_band_form_counts)


def crf_edits_band_scratch():
    """Private (scratch) bytes per lane of each banded form, keyed as `crf_edits_band_form_counts` keys them, as the runtime reports
    them for the loaded kernels (scrappie_hip_crf_edits_band_scratch; needs a GPU): the forms are built to need none."""
    return _edits_forms(lib().scrappie_hip_crf_edits_band_scratch, C.c_longlong)


def map_edits_form_counts():
    """The same for the transducer edit kernels, k_map_edits_rows and k_map_edits (scrappie_hip_map_edits_form_counts)."""
    return _edits_forms(lib().scrappie_hip_map_edits_form_counts)


def map_edits_band_form_counts():
    """Launches of each banded form of the transducer edit kernels in this process so far (scrappie_hip_map_edits_band_form_counts):
    {('rows', viterbi, tiled, backward): n, ('edits', viterbi, tiled, width): n}, width 256 or 64 positions per workgroup;
    `map_edits_form_counts` counts the unbanded forms alone."""
    return _edits_forms(lib().scrappie_hip_map_edits_band_form_counts, widths=(256, 64))


def map_edits_band_scratch():
    """Private (scratch) bytes per lane of each banded form, keyed as `map_edits_band_form_counts` keys them, as the runtime reports
    them for the loaded kernels (scrappie_hip_map_edits_band_scratch; needs a GPU): the forms are built to need none."""
    return _edits_forms(lib().scrappie_hip_map_edits_band_scratch, C.c_longlong, (256, 64))


def _edits_plan(seqlens, nblocks, plan):
    a = np.ascontiguousarray(seqlens, dtype=np.uintp)
    b = np.ascontiguousarray(nblocks, dtype=np.uintp)
    if len(a) != len(b):
        raise ValueError("one block count per sequence length")
    pitch = np.zeros(len(a), dtype=np.int32)
    rows, res = np.zeros(len(a), dtype=np.longlong), np.zeros(len(a), dtype=np.longlong)
    nres = C.c_longlong(0)
    sp, lp = C.POINTER(C.c_size_t), C.POINTER(C.c_longlong)
    nrow = plan(a.ctypes.data_as(sp), b.ctypes.data_as(sp), len(a), pitch.ctypes.data_as(C.POINTER(C.c_int)), rows.ctypes.data_as(lp),
                res.ctypes.data_as(lp), C.byref(nres))
    return pitch, rows, res, int(nrow), int(nres.value)


def crf_edits_plan(seqlens, nblocks):
    """The layout of one launch of the edit kernels over reads of `seqlens` bases and `nblocks` blocks (host arithmetic, no
    device; scrappie_hip_crf_edits_plan): (pitch, rows, res, row_floats, res_floats) -- per read the floats from one entry's
    row to the next, the float offset of its three row matrices (F_B, F_S, G_B, each (nblock + 1) * pitch floats) and of its
    9 L + 4 results; the floats of the two buffers."""
    return _edits_plan(seqlens, nblocks, lib().scrappie_hip_crf_edits_plan)


def _edits_band_row_bytes(fn, low, high, extra, what):
    """a read's row bytes in the band (low, high) of nblock + `extra` entries each"""
    lo, hi = (np.ascontiguousarray(x, dtype=np.uintp) for x in (low, high))
    if len(lo) != len(hi) or len(lo) < 1 + extra:
        raise ValueError("low and high hold %s entries each" % what)
    sp = C.POINTER(C.c_size_t)
    return int(fn(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), len(lo) - extra))


def _edits_band_plan(plan, seqlens, bands, extra, what, kmer_len=None, bandless=False):
    """`_edits_plan` for reads in bands of nblock + `extra` entries each; `bandless`: (nblock, None) is a read without a band"""
    bands = [b if bandless and b[1] is None else [np.ascontiguousarray(x, dtype=np.uintp) for x in b] for b in bands]
    if len(bands) != len(seqlens) or any(len(b) != 2 or (b[1] is not None and (len(b[0]) != len(b[1]) or len(b[0]) < 1 + extra)) for b in bands):
        raise ValueError("one (low, high) pair of %s entries each%s per sequence length" % (what, ", or (nblock, None)," if bandless else ""))
    sp = C.POINTER(C.c_size_t)
    n = len(bands)
    lo, hi = (sp * max(n, 1))(), (sp * max(n, 1))()
    for i, b in enumerate(bands):
        if b[1] is not None:
            lo[i], hi[i] = b[0].ctypes.data_as(sp), b[1].ctypes.data_as(sp)
    k = () if kmer_len is None else (kmer_len,)
    out = _edits_plan(seqlens, [int(b[0]) if b[1] is None else len(b[0]) - extra for b in bands], lambda a, nb, cnt, *rest: plan(a, nb, lo, hi, cnt, *k, *rest))
    if out[3] < 0:
        raise ValueError("a sequence of fewer than %d bases holds no k-mer" % kmer_len)
    return out


def crf_edits_band_row_bytes(low, high):
    """Device bytes of the three row matrices of a read in the band (low, high), nblock + 1 entries each
    (scrappie_hip_crf_edits_band_row_bytes): an entry's row holds its band's cells alone."""
    return _edits_band_row_bytes(lib().scrappie_hip_crf_edits_band_row_bytes, low, high, 1, "nblock + 1 >= 2")


def crf_edits_band_plan(seqlens, bands):
    """`crf_edits_plan` for reads in bands (scrappie_hip_crf_edits_band_plan): `bands[i]` is read i's (low, high), nblock + 1
    entries each -- the block count is the band's.  The pitch is that of the band's widest entry."""
    return _edits_band_plan(lib().scrappie_hip_crf_edits_band_plan, seqlens, bands, 1, "nblock + 1 >= 2")


def map_edits_plan(seqlens, nblocks, kmer_len):
    """The same for the transducer edit kernels and k-mers of `kmer_len` bases (scrappie_hip_map_edits_plan): two row matrices
    per read, F and G, of n + 1 = L - kmer_len + 2 floats per entry rounded up to 16.  ValueError where a sequence has fewer
    than `kmer_len` bases."""
    out = _edits_plan(seqlens, nblocks, lambda a, b, n, *rest: lib().scrappie_hip_map_edits_plan(a, b, n, kmer_len, *rest))
    if out[3] < 0:
        raise ValueError("a sequence of fewer than %d bases holds no k-mer" % kmer_len)
    return out


def map_edits_band_row_bytes(low, high):
    """Device bytes of the two row matrices of a transducer read in the band (low, high), nblock entries each
    (scrappie_hip_map_edits_band_row_bytes): an entry's row holds its band's cells alone."""
    return _edits_band_row_bytes(lib().scrappie_hip_map_edits_band_row_bytes, low, high, 0, "nblock >= 1")


def map_edits_band_plan(seqlens, bands, kmer_len):
    """`map_edits_plan` for reads in bands (scrappie_hip_map_edits_band_plan): `bands[i]` is read i's (low, high), nblock entries
    each -- the block count is the band's --, or (nblock, None) for a read without a band, which takes the unbanded pitch.  The
    pitch of a read in a band is that of the band's widest entry."""
    return _edits_band_plan(lib().scrappie_hip_map_edits_band_plan, seqlens, bands, 0, "nblock >= 1", kmer_len, True)


def _one_edits(seq, band, call):
    """what `map_post_edits` and `map_trans_edits` share once the matrix is checked: the results allocated, band(L) -- None for the
    call without a band, else `_one_band`'s -- handed to call(band, seq, L, base, sub, dele, ins); (base, sub, dele, ins)"""
    tgs, keep = _crf_targets([seq])
    L = len(keep[0])
    base = C.c_float(float('nan'))
    sub, dele, ins = (np.full(k, np.nan, dtype=np.float32) for k in (4 * L, max(L, 1), 4 * (L + 1)))
    fp = C.POINTER(C.c_float)
    if call(band(L), tgs[0].seq, L, C.byref(base), sub.ctypes.data_as(fp), dele.ctypes.data_as(fp), ins.ctypes.data_as(fp)) != 0:
        raise RuntimeError('An unknown error occurred while scoring edits: ' + last_error())
    return np.float32(base.value), sub.reshape(L, 4), dele[:L], ins.reshape(L + 1, 4)


def _one_band(lo, hi, entries, what, sane):
    """the band of a per-read edits call as pointers, checked: `entries` entries each, and sane(p_lo, p_hi)"""
    if len(lo) != entries or len(hi) != entries:
        raise ValueError('Supplied banding structure is not valid: %s entries each.' % what)
    p = tuple(x.ctypes.data_as(C.POINTER(C.c_size_t)) for x in (lo, hi))
    if not sane(*p):
        raise ValueError('Supplied banding structure is not valid.')
    return p + (lo, hi)      # (the arrays live as long as their pointers)


def map_post_edits(post, seq, stay_pen=0, skip_pen=0, local_pen=4.0, viterbi=True, bands=None):
    """Every single-base edit of `seq` (a base string, or an array of base codes 0..3) scored against a read's posterior under a
    transducer model (a `ScrappyMatrix` of 4^k + 1 log-probabilities per block, k = 1 .. 5, as `calc_post` gives) in one pass on
    the GPU (map_post_edits: a forward sweep, a backward sweep, one combining pass).  Returns (base, sub, dele, ins) numbered by
    `apply_edit` as `map_trans_edits` numbers them: base is `map_post_to_sequence`'s score of `seq` itself, bit for bit; the
    edits are what `map_post_to_sequence` gives for the edited sequence up to float32 rounding (confirm chosen edits with
    `map_post_to_sequences`, which is exact).  NaN: the edited sequence admits no path through the read or has fewer than k
    bases; everything is NaN, and `last_error()` says why, where `seq` cannot be scored (empty, shorter than a k-mer, not bases,
    too long for k_map_edits).
    `bands`: None, an int (scrappy's `diagonal_bands` over the n = len(seq) - k + 1 states, as `map_post_to_sequence` reads it) or a
    (low, high) pair of nblock entries each, from `map_path_band` for one: the edits are scored inside the band
    (map_post_edits_banded) -- every state of the original sequence keeps its band, the edit's own new states are free; base is then
    the score of the masked programme, which is NOT `map_post_to_sequence(..., bands=bands)`'s (that keeps the reference's stale
    cells); a band that is not valid is a ValueError."""
    if not isinstance(post, ScrappyMatrix):
        raise TypeError('`post` should be a ScrappyMatrix.')
    nblock, nstate = post.shape
    if nstate not in (5, 17, 65, 257, 1025):
        raise ValueError('`post` should hold 4^k + 1 states per block, k = 1 .. 5.')
    kmer_len = guess_state_properties(nstate)[1]

    def band(L):
        if bands is None or L < kmer_len:
            return None
        n = L - kmer_len + 1
        return _one_band(*_map_band(bands, nblock, n), nblock, 'nblock', lambda lo, hi: lib().are_bounds_sane(lo, hi, nblock, n))

    def call(b, seq, L, *out):
        if b is None:
            return lib().map_post_edits(post.data(), stay_pen, skip_pen, local_pen, seq, L, 1 if viterbi else 0, *out)
        return lib().map_post_edits_banded(post.data(), stay_pen, skip_pen, local_pen, seq, L, b[0], b[1], 1 if viterbi else 0, *out)
    return _one_edits(seq, band, call)


def map_trans_edits(trans, seq, viterbi=True, bands=None):
    """Every single-base edit of `seq` (a base string, or an array of base codes 0..3) scored against a read's transitions
    under a flip-flop (CRF) model (a `ScrappyMatrix` of 25 rows, as `calc_post(rt, model='rnnrf_r94')` gives) in one pass on
    the GPU (map_crf_edits: a forward sweep, a backward sweep, one combining pass).  Returns (base, sub, dele, ins): base is
    `map_trans_to_sequence`'s score of `seq` itself, bit for bit; sub (L, 4), dele (L,) and ins (L + 1, 4) are float32 arrays,
    sub[i][c], dele[i] and ins[i][c] what `map_trans_to_sequence` gives for `apply_edit(seq, 'sub' / 'del' / 'ins', i, c)` up to
    float32 rounding (an edit's score and base are different chains of additions: confirm chosen edits with
    `map_trans_to_sequences`, which is exact).  NaN: the edited sequence has more bases than the read has entries, or is empty;
    everything is NaN, and `last_error()` says why, where `seq` cannot be scored (empty, not bases, too long for k_crf_edits).
    `bands`: None, an int (half-width in cells of the diagonal band, as `map_trans_to_sequence` reads it) or a (low, high) pair of
    nblock + 1 entries each, from `map_crf_path_band` for one: the edits are scored inside the band (map_crf_edits_banded) --
    every cell of the original sequence keeps its band, the new base's own cell is free; base is then
    `map_trans_to_sequence(..., bands=bands)`'s score; a band that is not valid is a ValueError."""
    if not isinstance(trans, ScrappyMatrix):
        raise TypeError('`trans` should be a ScrappyMatrix.')
    nblock, nstate = trans.shape
    if nstate != 25:
        raise ValueError('`trans` should hold the 25 transitions of a flip-flop (CRF) model per block.')

    def band(L):
        if bands is None or L == 0:
            return None
        return _one_band(*_crf_band(bands, nblock, L), nblock + 1, 'nblock + 1', lambda lo, hi: lib().scrappie_hip_map_crf_bounds_sane(lo, hi, nblock, L))

    def call(b, seq, L, *out):
        if b is None:
            return lib().map_crf_edits(trans.data(), seq, L, 1 if viterbi else 0, *out)
        return lib().map_crf_edits_banded(trans.data(), seq, L, b[0], b[1], 1 if viterbi else 0, *out)
    return _one_edits(seq, band, call)


def map_trans_to_reference(trans, sequence, viterbi=False, path=False):
    """Where in `sequence` does this read lie?  A read's transitions under a flip-flop (CRF) model (a `ScrappyMatrix` of 25
    rows, as `calc_post(rt, model='rnnrf_r94')` gives) mapped INTO a longer base sequence: the paths of `map_trans_to_sequence`
    that begin and end anywhere in it; the DP runs on the GPU, one workgroup per window of the sequence (k_map_crf_local).
    Returns (score, first, last, path): the read spells sequence[first:last]; path[t], t = 0 .. nblock, is the index in
    `sequence` of the last base emitted through entry t (first - 1 while none).  Forward: (score, None, None, None); Viterbi
    without `path`: (score, None, last, None) -- the start is known only from the traceback."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(trans, ScrappyMatrix):
        raise TypeError('`trans` should be a ScrappyMatrix.')
    nblock, nstate = trans.shape
    if nstate != 25:
        raise ValueError('`trans` should hold the 25 transitions of a flip-flop (CRF) model per block.')
    codes = encode_bases(sequence, 1).astype(np.int32)
    p_seq = codes.ctypes.data_as(C.POINTER(C.c_int))
    if not viterbi:
        score = lib().map_crf_to_reference_forward(trans.data(), p_seq, len(codes))
        if np.isnan(score):
            raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
        return score, None, None, None
    first, last = C.c_size_t(0), C.c_size_t(0)
    path_data = np.zeros(nblock + 1, dtype=np.int32) if path else None
    score = lib().map_crf_to_reference_viterbi(trans.data(), p_seq, len(codes), C.byref(first) if path else None, C.byref(last),
                                               path_data.ctypes.data_as(C.POINTER(C.c_int)) if path else None)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score, (int(first.value) if path else None), int(last.value), path_data


def map_post_to_reference(post, sequence, stay_pen=0, skip_pen=0, local_pen=4.0, viterbi=False, path=False):
    """Where in `sequence` does this read lie?  A posterior of a transducer model (a `ScrappyMatrix` of log-probabilities, as
    from `calc_post`) mapped INTO a longer base sequence: `map_post_to_sequence` with the sequence side made local -- the path
    may enter the sequence from START at any position and leave it for END from any position; the DP runs on the GPU, one
    workgroup per window of the sequence (k_map_local).  Returns (score, first, last, path): `first` is the lowest k-mer
    position the path visits and `last` the highest plus one, so the read spells sequence[first:last + k - 1]; path[blk],
    nblock entries, is the position or -1 in START / END.  Forward: (score, None, None, None); Viterbi without `path`:
    (score, None, last, None) -- the start is known only from the traceback."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(post, ScrappyMatrix):
        raise TypeError('`post` should be a ScrappyMatrix.')
    nblock, nstate = post.shape
    kmer_len = guess_state_properties(nstate)[1]
    codes = np.ascontiguousarray(encode_bases(sequence, kmer_len), dtype=np.int32)
    p_seq = codes.ctypes.data_as(C.POINTER(C.c_int))
    if not viterbi:
        score = lib().map_to_reference_forward(post.data(), stay_pen, skip_pen, local_pen, p_seq, len(codes))
        if np.isnan(score):
            raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
        return score, None, None, None
    first, last = C.c_size_t(0), C.c_size_t(0)
    path_data = np.zeros(nblock, dtype=np.int32) if path else None
    score = lib().map_to_reference_viterbi(post.data(), stay_pen, skip_pen, local_pen, p_seq, len(codes), C.byref(first) if path else None,
                                           C.byref(last), path_data.ctypes.data_as(C.POINTER(C.c_int)) if path else None)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score, (int(first.value) if path else None), int(last.value), path_data


def _motif_targets(motifs, strict):
    """The ctypes scrappie_hip_map_target array of `motifs` (base strings, or arrays of base codes 0..3) and what keeps its memory
    alive.  strict: an empty motif or a base outside ACGT raises ValueError; otherwise it becomes an empty motif, which the
    library answers with NaN."""
    tgs = (_MapTarget * max(len(motifs), 1))()
    keep = []
    for i, sq in enumerate(motifs):
        try:
            if isinstance(sq, str):
                if len(sq) == 0:
                    raise ValueError("an empty motif")
                codes = np.ascontiguousarray(encode_bases(sq, 1), dtype=np.int32)
            else:
                codes = np.ascontiguousarray(sq, dtype=np.int32)
                if len(codes) == 0 or codes.min() < 0 or codes.max() > 3:
                    raise ValueError("a motif holds base codes 0..3 and at least one of them")
        except ValueError:
            if strict:
                raise
            codes = np.zeros(0, dtype=np.int32)
        keep.append(codes)
        tgs[i].seq = codes.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(codes)
    return tgs, keep


def find_in_trans(trans, motifs, positions=True):
    """Do these short sequences occur INSIDE this read?  A read's transitions under a flip-flop (CRF) model (a `ScrappyMatrix` of
    25 rows, as `calc_post(rt, model='rnnrf_r94')` gives) searched for each of `motifs` (base strings -- a barcode, an adapter,
    a primer): the best path of the whole read whose bases between two entries `begin` <= `end` spell the motif exactly, the
    entries before and behind them free; Viterbi, on the GPU, the motifs packed into workgroups (k_crf_find).  Returns
    (scores, call_score, begins, ends): float32 scores, NaN where a motif cannot be searched (longer than the read's nblock + 1
    entries, or than k_crf_find holds: `last_error()` says which); call_score, decode_crf's score of the read, so that
    scores - call_score <= 0 are log-odds against the read's own call, 0 where the motif is a run of the call's bases; begins and
    ends (int32, -1 beside a NaN; None without `positions`) are entries of the path, 0 .. nblock: entry t lies at sample
    t * stride of the signal the transitions were computed from (stride: the model's convolution stride), so the motif covers
    samples [begin * stride, (end + 1) * stride).  The motif is searched as given: for the other strand pass its reverse
    complement as another motif."""
    if not isinstance(trans, ScrappyMatrix):
        raise TypeError('`trans` should be a ScrappyMatrix.')
    nblock, nstate = trans.shape
    if nstate != 25:
        raise ValueError('`trans` should hold the 25 transitions of a flip-flop (CRF) model per block.')
    motifs = list(motifs)
    n = len(motifs)
    tgs, keep = _motif_targets(motifs, True)
    score = np.full(max(n, 1), np.nan, dtype=np.float32)
    begin, end = (np.full(max(n, 1), -1, dtype=np.int32) for _ in range(2)) if positions else (None, None)
    call = C.c_float(float('nan'))
    i32 = C.POINTER(C.c_int32)
    if lib().find_crf_sequences_viterbi(trans.data(), tgs, n, score.ctypes.data_as(C.POINTER(C.c_float)),
                                        begin.ctypes.data_as(i32) if positions else None, end.ctypes.data_as(i32) if positions else None,
                                        C.byref(call)) != 0:
        raise RuntimeError('An unknown error occurred during the search: ' + last_error())
    return score[:n], np.float32(call.value), (begin[:n] if positions else None), (end[:n] if positions else None)


_squiggle_fn_ = {
    'squiggle_r94': 'squiggle_r94',
    'squiggle_r94_rna': 'squiggle_r94_rna',
    'squiggle_r10': 'squiggle_r10',
}


def _base_codes(sequence):
    """the bases of `sequence` coded 0..3 as an int32 array (encode_bases_to_integers with a state of one base)"""
    return encode_bases(sequence, 1).astype(np.int32)


def sequence_to_squiggle(sequence, model='squiggle_r94', rescale=False):
    """python/scrappy/__init__.py:433-459: the squiggle a base sequence is predicted to give, a `ScrappyMatrix` of
    len(sequence) columns of (mean, log sd, dwell logit); with rescale, (mean, sd, expected dwell).  The network runs on
    the GPU; `model` must have been registered (`register_model`): no weights are compiled in."""
    try:
        fn = getattr(lib(), _squiggle_fn_[model])
    except KeyError:
        raise KeyError("Squiggle model '{}' not recognised.".format(model))
    ptr = lib().encode_bases_to_integers(sequence.encode(), len(sequence), 1)
    if not ptr:
        raise RuntimeError('An unknown error occurred whilst encoding sequence: ' + last_error())
    try:
        squiggle = fn(C.cast(ptr, C.POINTER(C.c_int)), len(sequence), rescale)
    finally:
        _libc.free(ptr)
    if not squiggle:
        raise RuntimeError('An unknown error occurred whilst generating squiggle: ' + last_error())
    return ScrappyMatrix(squiggle)


def _squiggle_matrix(squiggle, model=None):
    """a predicted squiggle as a ScrappyMatrix of npos columns (mean, log sd, dwell logit): one as it is, an (npos, 3)
    array converted, a base sequence predicted with the squiggle model `model`"""
    if isinstance(squiggle, str):
        if model is None:
            raise NotImplementedError("a base sequence needs the name of a registered squiggle model (model='squiggle_r94', "
                                      "...; no weights are compiled in); or pass the predicted squiggle, a ScrappyMatrix or "
                                      "an (npos, 3) array of (mean, log sd, dwell logit)")
        return sequence_to_squiggle(squiggle, model=model, rescale=False)
    if isinstance(squiggle, ScrappyMatrix):
        return squiggle
    a = np.asarray(squiggle, dtype=ftype)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError("`squiggle` should be a ScrappyMatrix or an (npos, 3) array.")
    return ScrappyMatrix.from_numpy(a, sloika=False)


def squiggle_match(rt, squiggle, rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0, min_score=5.0, viterbi=True,
                   path=True, band=None):
    """squiggle_match_viterbi / squiggle_match_forward (decode.c:1035, :1262) on the GPU: the `RawTable` rt as it is (no
    trimming), mapped over [rt.start, rt.end), against a predicted squiggle.  Returns (score, path or None); the path has
    rt's full length, -1 outside the window and in the START / END states.  `band`: None, an int (the half-width in
    positions of a diagonal band, `squiggle_diagonal_band`) or a (low, width) pair -- low[t] the first position sample t of
    the window may map to, width how many (squiggle_match_viterbi_banded / _forward_banded)."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(rt, RawTable):
        raise TypeError('`rt` should be a RawTable.')
    sq = _squiggle_matrix(squiggle)
    i32p = C.POINTER(C.c_int32)
    if band is not None:
        low, width = _squiggle_band(band, max(int(rt._rt.end) - int(rt._rt.start), 0), int(sq.data().contents.nc))
        lowp = low.ctypes.data_as(i32p) if low is not None else None
    if viterbi:
        path_data = np.zeros(rt._rt.n, dtype=np.int32)
        if band is None:
            score = lib().squiggle_match_viterbi(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score,
                                                 path_data.ctypes.data_as(i32p))
        else:
            score = lib().squiggle_match_viterbi_banded(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score,
                                                        lowp, width, path_data.ctypes.data_as(i32p))
    else:
        path_data = None
        if band is None:
            score = lib().squiggle_match_forward(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score)
        else:
            score = lib().squiggle_match_forward_banded(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score, lowp, width)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    return score, (path_data if path else None)


def squiggle_match_reference(rt, squiggle, rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0, min_score=5.0, viterbi=True,
                             path=False):
    """Where inside a longer reference squiggle does this signal lie?  (squiggle_match_local_viterbi / _forward, k_squig_local; not
    in the reference project.)  The `RawTable` rt as it is, mapped over [rt.start, rt.end), INTO `squiggle` (a ScrappyMatrix or an
    (npos, 3) array): entering and leaving the squiggle is free at every position.  Returns (score, first, last, path): `last` is
    the position the path ends in, or left the squiggle from, plus one (None without viterbi); `first`, the lowest position on
    the path, and the path (rt's full length; positions in the squiggle's coordinates, -1 outside the window and in START / END)
    need `path` and are None without it."""
    _path_needs_viterbi(path, viterbi)
    if not isinstance(rt, RawTable):
        raise TypeError('`rt` should be a RawTable.')
    sq = _squiggle_matrix(squiggle)
    if viterbi:
        path_data = np.zeros(rt._rt.n, dtype=np.int32) if path else None
        first, last = C.c_size_t(0), C.c_size_t(0)
        score = lib().squiggle_match_local_viterbi(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score,
                                                   path_data.ctypes.data_as(C.POINTER(C.c_int32)) if path else None,
                                                   C.byref(first) if path else None, C.byref(last))
    else:
        score = lib().squiggle_match_local_forward(rt.data(), rate, sq.data(), back_prob, local_pen, skip_pen, min_score)
    if np.isnan(score):
        raise RuntimeError('An unknown error occurred during alignment: ' + last_error())
    if not viterbi:
        return score, None, None, None
    return score, (int(first.value) if path else None), int(last.value), path_data


def map_signal_to_squiggle(data, squiggle, rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0, min_score=5.0, model=None,
                           band=None):
    """python/scrappy/__init__.py:462-489: `squiggle` is a base sequence, predicted with the registered squiggle model
    `model`, or the predicted squiggle itself (a `ScrappyMatrix` or an (npos, 3) array); then trim -> scale ->
    squiggle_match_viterbi.  Returns (score, path over the whole of `data`).  `band`: as `squiggle_match` takes it, over
    the trimmed window."""
    sq = _squiggle_matrix(squiggle, model)
    raw = RawTable(data)
    raw.trim().scale()
    return squiggle_match(raw, sq, rate, back_prob, local_pen, skip_pen, min_score, viterbi=True, path=True, band=band)


def plan_tail(lengths, stride, max_long_blocks=0):
    """scrappie_hip_plan_tail (host only): boolean array, True for the chain-bound reads a call runs beside the others"""
    ln = np.ascontiguousarray(lengths, dtype=np.uint32)
    flags = np.zeros(len(ln), np.uint8)
    L = lib()
    L.scrappie_hip_plan_tail.restype = C.c_long
    L.scrappie_hip_plan_tail.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_ubyte)]
    n = L.scrappie_hip_plan_tail(ln.ctypes.data_as(C.POINTER(C.c_uint32)), len(ln), stride, max_long_blocks, flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if n < 0:
        raise RuntimeError("plan_tail: invalid arguments")
    assert int(flags.sum()) == n
    return flags.astype(bool)


def plan_dynamic(lengths, stride, nengine, max_reads=16384, max_blocks=0):
    """The hand-out plan of basecall_multi (host only): (order, starts): read indices sorted by length,
    longest first, and the first position of each launch group in that order."""
    ln = np.ascontiguousarray(lengths, dtype=np.uint32)
    n = len(ln)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    starts = np.zeros(max(n, 1), dtype=np.uintp)
    ng = lib().scrappie_hip_plan_dynamic(ln.ctypes.data_as(C.POINTER(C.c_uint32)), n, stride, nengine, max_reads, max_blocks,
                                         order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         starts.ctypes.data_as(C.POINTER(C.c_size_t)), len(starts))
    if ng < 0:
        raise RuntimeError("plan_dynamic: a read alone exceeds max_blocks")
    return order[:n], starts[:ng]


def basecall_multi(engines, signals, model='rgrgr_r94', params=None):
    """scrappie_hip_basecall_batch_multi: `signals` spread over several engines (one per GPU), launch groups
    handed out from an atomic cursor over the reads sorted by length.  Returns the calls in input order."""
    n = len(signals)
    p = params or engines[0].default_params()
    keep = [np.ascontiguousarray(s, dtype=ftype) for s in signals]
    rts = (_RawTable * max(n, 1))()
    for i, s in enumerate(keep):
        rts[i] = _RawTable(None, len(s), 0, len(s), s.ctypes.data_as(C.POINTER(C.c_float)))
    calls = (_Call * max(n, 1))()
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    ms = (C.c_int * len(engines))(*[e._models[model] for e in engines])
    if lib().scrappie_hip_basecall_batch_multi(hs, ms, len(engines), rts, n, C.byref(p), calls) != 0:
        raise RuntimeError("basecall_batch_multi: " + last_error())
    return Engine._unpack(calls, n, p.want_pos)


class Prep(object):
    """Signal preparation of a batch on the device (scrappie_hip_prep_*, k_p0): trim_and_segment_raw +
    medmad_normalise_array of the reference (scrappie_raw.c:270-277) for every read of a batch in one launch."""

    def __init__(self, device=0):
        self._h = lib().scrappie_hip_prep_create(device)
        if not self._h:
            raise RuntimeError("prep_create: " + last_error())

    def close(self):
        if self._h:
            lib().scrappie_hip_prep_destroy(self._h)
            self._h = None

    def run(self, raws, trim_start=200, trim_end=10, varseg_chunk=100, varseg_thresh=0.0, slot=0, windows=None, stage_capacity=None):
        """raws: list of float32 arrays of RAW samples (windows: optional list of (start, end) at entry).
        stage_capacity (samples): place the reads in the slot's pinned staging buffer first, as a loader does
        (scrappie_hip_prep_begin / _alloc); the ones that do not fit stay where they are and are gathered by the call.
        Returns (device pointer, offsets, lengths, start, end): offsets / lengths as run_device / basecall_device take them."""
        n = len(raws)
        self._keep = [np.ascontiguousarray(r, dtype=ftype) for r in raws]
        rts = (_RawTable * max(n, 1))()
        ctx = None
        self.n_staged = 0
        if stage_capacity is not None:
            ctx = lib().scrappie_hip_prep_begin(self._h, slot, int(stage_capacity))
            if not ctx:
                raise RuntimeError("prep_begin: " + last_error())
        for i, r in enumerate(self._keep):
            st, en = windows[i] if windows is not None else (0, len(r))
            ptr = lib().scrappie_hip_prep_alloc(ctx, len(r)) if ctx else None
            if ptr:
                C.memmove(ptr, r.ctypes.data, r.nbytes)
                assert lib().scrappie_hip_prep_owns(self._h, slot, ptr) == 1
                self.n_staged += 1
                rts[i] = _RawTable(None, len(r), st, en, C.cast(ptr, C.POINTER(C.c_float)))
                continue
            rts[i] = _RawTable(None, len(r), st, en, r.ctypes.data_as(C.POINTER(C.c_float)))
        d = C.c_void_p()
        off = np.zeros(max(n, 1), np.uint64); ln = np.zeros(max(n, 1), np.uint32)
        st = np.zeros(max(n, 1), np.uint32); en = np.zeros(max(n, 1), np.uint32)
        u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        if lib().scrappie_hip_prep_run(self._h, slot, rts, n, trim_start, trim_end, varseg_chunk, varseg_thresh, C.byref(d),
                                       off.ctypes.data_as(u64), ln.ctypes.data_as(u32), st.ctypes.data_as(u32), en.ctypes.data_as(u32)) != 0:
            raise RuntimeError("prep_run: " + last_error())
        return d.value, off[:n], ln[:n], st[:n], en[:n]

    def fetch(self, offset, count, slot=0):
        out = np.empty(int(count), ftype)
        if count and lib().scrappie_hip_prep_fetch(self._h, slot, int(offset), int(count), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            raise RuntimeError("prep_fetch: " + last_error())
        return out

    def timing(self, slot=0):
        t = (C.c_double * 3)()
        lib().scrappie_hip_prep_timing(self._h, slot, t)
        return {"gather_ms": t[0], "h2d_ms": t[1], "k_p0_ms": t[2]}


def _score_edits(eng, fn, name, signals, sequences, model, viterbi, bands=None, kmer_len=0, **params):
    """one batch call of an edits engine: a shared sequence is encoded once; [(base, sub, dele, ins)].  `bands`: None, or per read
    None, an int or a (low, high) pair; the library reads nblock + 1 entries of each array (a transducer model, `kmer_len` -1 -- the
    model's own, asked of the engine once the arguments have passed --: nblock entries, over the L - kmer_len + 1 states), so a pair
    of any other length goes in as that many entries of an empty band, which it refuses for that read."""
    n = len(signals)
    if isinstance(sequences, str) or (len(sequences) and np.ndim(sequences[0]) == 0 and not isinstance(sequences[0], str)):
        sequences = [sequences] * n
    sequences = list(sequences)
    if len(sequences) != n:
        raise ValueError("one sequence for all signals, or one sequence per signal")
    h = eng._models[model]
    if kmer_len < 0:
        nstate = lib().scrappie_hip_model_states(eng._h, h)
        kmer_len = 1 if nstate == 25 else guess_state_properties(nstate)[1]      # (a flip-flop model: refused by the library)
    rts, keep = _raw_tables(signals)
    made = {}
    tgs = (_MapTarget * max(n, 1))()
    for i, sq in enumerate(sequences):
        if id(sq) not in made:
            made[id(sq)] = _crf_targets([sq])
        tgs[i].seq, tgs[i].seqlen = made[id(sq)][0][0].seq, made[id(sq)][0][0].seqlen
    if bands is not None:
        for i, b in enumerate(bands):
            nblock, L = eng.read_blocks(model, len(keep[i])), int(tgs[i].seqlen)
            if b is None or nblock <= 0 or L == 0 or L < kmer_len:      # (a read too short or a sequence that holds nothing is refused by the library as it is)
                continue
            nent = nblock if kmer_len else nblock + 1
            lo, hi = _map_band(b, nblock, L - kmer_len + 1) if kmer_len else _crf_band(b, nblock, L)
            if len(lo) != nent or len(hi) != nent:
                lo, hi = np.zeros(nent, dtype=np.uintp), np.zeros(nent, dtype=np.uintp)
            keep += [lo, hi]
            tgs[i].poslow = lo.ctypes.data_as(C.POINTER(C.c_size_t))
            tgs[i].poshigh = hi.ctypes.data_as(C.POINTER(C.c_size_t))
    p = eng.default_params(**params)
    out = (_EditsResult * max(n, 1))()
    if fn(eng._h, h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, out) != 0:
        raise RuntimeError(name + ": " + last_error())
    res = []
    take = lambda q, k: np.ctypeslib.as_array(q, shape=(k,)).copy() if k else np.zeros(0, dtype=np.float32)
    for r in (out[i] for i in range(n)):
        L = int(r.seqlen)
        res.append((np.float32(r.base), take(r.sub, 4 * L).reshape(L, 4), take(r.dele, L), take(r.ins, 4 * (L + 1)).reshape(L + 1, 4)))
    lib().scrappie_hip_free_edits_results(out, n)
    return res


class Engine(object):
    """One GPU.  `basecall(signals)` takes a list of trimmed, normalised float32
    arrays and returns a list of dicts (bases, score, nblock[, pos]); reads are
    coalesced into launch groups, decoded on device."""

    def __init__(self, device=0):
        self._h = lib().scrappie_hip_engine_create(device)
        if not self._h:
            raise RuntimeError("engine_create(%d): %s" % (device, last_error()))
        self.device = device
        self._models = {}

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_alt_dev", None):
                self.set_decoder_input(None)
            if getattr(self, "_trk_dev", None):
                self.set_trunk_input(None)
            lib().scrappie_hip_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def load_model(self, name, weights):
        """`weights` is a model dict (scrappie_amd.model) or a path to a .scrm file."""
        if isinstance(weights, dict):
            import tempfile
            with tempfile.NamedTemporaryFile(suffix=".scrm", delete=False) as fh:
                path = fh.name
            try:
                _model.save_model(weights, path)
                h = lib().scrappie_hip_load_model(self._h, name.encode(), os.fsencode(path))
            finally:
                os.unlink(path)
        else:
            h = lib().scrappie_hip_load_model(self._h, name.encode(), os.fsencode(weights))
        if h < 0:
            raise RuntimeError("load_model(%s): %s" % (name, last_error()))
        self._models[name] = h
        return h

    def default_params(self, **kw):
        p = lib().scrappie_hip_default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def min_samples(self, model):
        return lib().scrappie_hip_min_samples(self._h, self._models[model])

    def set_profiling(self, on=True):
        lib().scrappie_hip_set_profiling(self._h, 1 if on else 0)

    def set_max_launch_reads(self, n):
        lib().scrappie_hip_set_max_launch_reads(self._h, n)

    def set_max_launch_blocks(self, n):
        lib().scrappie_hip_set_max_launch_blocks(self._h, n)

    def timing(self):
        t = Timing()
        lib().scrappie_hip_get_timing(self._h, C.byref(t))
        return {f[0]: getattr(t, f[0]) for f in Timing._fields_}

    @staticmethod
    def _unpack(calls, n, want_pos):
        out = []
        for i in range(n):
            c = calls[i]
            if not c.basecall:
                out.append(None)
                continue
            d = dict(bases=C.string_at(c.basecall).decode(), score=float(c.score), nblock=int(c.nblock))
            if want_pos and c.pos:
                d["pos"] = np.ctypeslib.as_array(c.pos, shape=(c.nblock + 1,)).copy()
            out.append(d)
        lib().scrappie_hip_free_calls(calls, n)
        return out

    def basecall(self, signals, model='rgrgr_r94', params=None, base_probs=False):
        """base_probs (CRF models only): every call gains "base_probs", the (nblock + 1, 5) float32 posterior over A, C, G, T and stay
        at every block boundary, in the orientation `basecall_raw(..., with_base_probs=True)` returns (scrappie_hip_basecall_batch_probs)."""
        if base_probs:
            return self._basecall_probs(signals, model, params)
        n = len(signals)
        p = params or self.default_params()
        keep = [np.ascontiguousarray(s, dtype=ftype) for s in signals]
        rts = (_RawTable * n)()
        for i, s in enumerate(keep):
            rts[i] = _RawTable(None, len(s), 0, len(s), s.ctypes.data_as(C.POINTER(C.c_float)))
        calls = (_Call * n)()
        if lib().scrappie_hip_basecall_batch(self._h, self._models[model], rts, n, C.byref(p), calls) != 0:
            raise RuntimeError("basecall_batch: " + last_error())
        return self._unpack(calls, n, p.want_pos)

    def _basecall_probs(self, signals, model, params):
        h = self._models[model]
        if lib().scrappie_hip_model_states(self._h, h) != 25:
            raise ValueError("Base probabilities not supported for model type '{}': a CRF model is needed.".format(model))
        n = len(signals)
        p = params or self.default_params()
        rts, keep = _raw_tables(signals)
        calls = (_Call * max(n, 1))()
        probs = (C.POINTER(_Mat) * max(n, 1))()
        if lib().scrappie_hip_basecall_batch_probs(self._h, h, rts, n, C.byref(p), calls, probs) != 0:
            raise RuntimeError("basecall_batch_probs: " + last_error())
        mats = [ScrappyMatrix(probs[i]).data(as_numpy=True, sloika=False) if probs[i] else None for i in range(n)]
        out = self._unpack(calls, n, p.want_pos)
        for d, bp in zip(out, mats):
            if d is not None:
                d["base_probs"] = bp
        return out

    def posterior_crf(self, transitions):
        """The base probabilities of each read's transitions, batched (scrappie_hip_posterior_crf_batch): `transitions` holds
        `ScrappyMatrix` objects or (nblock, 25) arrays as `calc_post(rt, 'rnnrf_r94').data(as_numpy=True, sloika=False)` gives them;
        returns a list of (nblock + 1, 5) float32 arrays in input order, None where a matrix is refused (`last_error()` says why)."""
        n = len(transitions)
        keep, ptrs = [], (C.POINTER(_Mat) * max(n, 1))()
        for i, t in enumerate(transitions):
            if isinstance(t, ScrappyMatrix):
                keep.append(t)
            else:
                a = np.asarray(t, dtype=ftype)
                if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
                    keep.append(None)       # the library refuses a null matrix
                    continue
                keep.append(ScrappyMatrix.from_numpy(a, sloika=False))
            ptrs[i] = keep[-1].data()
        out = (C.POINTER(_Mat) * max(n, 1))()
        if lib().scrappie_hip_posterior_crf_batch(self._h, ptrs, n, out) != 0:
            raise RuntimeError("posterior_crf_batch: " + last_error())
        return [ScrappyMatrix(out[i]).data(as_numpy=True, sloika=False) if out[i] else None for i in range(n)]

    def crf_post_timing(self):
        """the last base-probability call's time (ms, summed over launch groups).  basecall(base_probs=True): network + k_crf, k_crf_post,
        the probabilities' transfer; posterior_crf: staging + upload, k_crf_post, download + results"""
        return self._timing(lib().scrappie_hip_crf_post_timing, ('network_ms', 'post_ms', 'download_ms'))

    # -- device-resident path (bench) ------------------------------------
    def basecall_deferred(self, signals, model='rgrgr_r94', params=None):
        """scrappie_hip_basecall_batch_deferred: (calls, ticket, deferred) -- calls[i] is None where deferred[i]; pass the returned
        ticket to collect_deferred() (the signals are kept alive with it)."""
        n = len(signals)
        p = params or self.default_params()
        keep = [np.ascontiguousarray(s, dtype=ftype) for s in signals]
        rts = (_RawTable * max(n, 1))()
        for i, s in enumerate(keep):
            rts[i] = _RawTable(None, len(s), 0, len(s), s.ctypes.data_as(C.POINTER(C.c_float)))
        calls = (_Call * max(n, 1))()
        flags = np.zeros(max(n, 1), np.uint8)
        L = lib()
        L.scrappie_hip_basecall_batch_deferred.restype = C.c_long
        L.scrappie_hip_basecall_batch_deferred.argtypes = [C.c_void_p, C.c_int, C.POINTER(_RawTable), C.c_size_t, C.POINTER(Params),
                                                           C.POINTER(_Call), C.POINTER(C.c_ubyte)]
        tk = L.scrappie_hip_basecall_batch_deferred(self._h, self._models[model], rts, n, C.byref(p), calls, flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if tk < 0:
            raise RuntimeError("basecall_batch_deferred: " + last_error())
        out = Engine._unpack(calls, n, p.want_pos)
        deferred = flags[:n].astype(bool)
        if tk > 0:
            self._deferred = getattr(self, "_deferred", {})
            self._deferred[tk] = (keep, rts, int(deferred.sum()), p.want_pos)
        return out, tk, deferred

    def basecall_device_deferred(self, dptr, offsets, lengths, model='rgrgr_r94', params=None):
        """scrappie_hip_basecall_device_deferred on signals already in HBM (e.g. from Prep.run): (calls, ticket, deferred) as above;
        the device buffer may be reused as soon as this returns."""
        p = params or self.default_params()
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        n = len(ln)
        calls = (_Call * max(n, 1))()
        flags = np.zeros(max(n, 1), np.uint8)
        L = lib()
        L.scrappie_hip_basecall_device_deferred.restype = C.c_long
        L.scrappie_hip_basecall_device_deferred.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t,
                                                            C.POINTER(Params), C.POINTER(_Call), C.POINTER(C.c_ubyte)]
        tk = L.scrappie_hip_basecall_device_deferred(self._h, self._models[model], dptr, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     ln.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(p), calls,
                                                     flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if tk < 0:
            raise RuntimeError("basecall_device_deferred: " + last_error())
        out = Engine._unpack(calls, n, p.want_pos)
        deferred = flags[:n].astype(bool)
        if tk > 0:
            self._deferred = getattr(self, "_deferred", {})
            self._deferred[tk] = (None, None, int(deferred.sum()), p.want_pos)
        return out, tk, deferred

    def collect_deferred(self, ticket, wait=True):
        """the calls of a ticket's deferred reads in their call's order; None if wait is False and they are not ready"""
        keep, rts, nl, want_pos = self._deferred[ticket]
        calls = (_Call * max(nl, 1))()
        L = lib()
        L.scrappie_hip_deferred_collect.restype = C.c_long
        L.scrappie_hip_deferred_collect.argtypes = [C.c_void_p, C.c_long, C.POINTER(_Call), C.c_size_t, C.c_int]
        k = L.scrappie_hip_deferred_collect(self._h, ticket, calls, nl, 1 if wait else 0)
        if k == -2:
            return None
        del self._deferred[ticket]
        if k < 0:
            raise RuntimeError("deferred_collect: " + last_error())
        return Engine._unpack(calls, k, want_pos)

    def upload(self, flat_signal):
        flat = np.ascontiguousarray(flat_signal, dtype=ftype)
        d = lib().scrappie_hip_device_alloc(self._h, flat.nbytes)
        if not d:
            raise RuntimeError("device_alloc: " + last_error())
        if lib().scrappie_hip_memcpy_h2d(self._h, d, flat.ctypes.data, flat.nbytes) != 0:
            raise RuntimeError("memcpy_h2d: " + last_error())
        return d

    def free(self, dptr):
        lib().scrappie_hip_device_free(self._h, dptr)

    def run_device(self, dptr, offsets, lengths, model='rgrgr_r94', params=None):
        """Launch the device pipeline on reads already in HBM; returns #blocks."""
        p = params or self.default_params()
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        r = lib().scrappie_hip_run_device(self._h, self._models[model], dptr,
                                          off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          ln.ctypes.data_as(C.POINTER(C.c_uint32)), len(ln), C.byref(p))
        if r < 0:
            raise RuntimeError("run_device: " + last_error())
        return r

    def collect(self, n, params=None, raw=False):
        p = params or self.default_params()
        calls = (_Call * n)()
        if lib().scrappie_hip_collect(self._h, C.byref(p), calls, n) != 0:
            raise RuntimeError("collect: " + last_error())
        if raw:     # bench: only count bases, then free
            nb = int(np.frombuffer(calls, dtype=np.uint64).reshape(n, C.sizeof(_Call) // 8)[:, 3].sum()) if n else 0
            lib().scrappie_hip_free_calls(calls, n)
            return nb
        return self._unpack(calls, n, p.want_pos)

    def synchronize(self):
        lib().scrappie_hip_synchronize(self._h)

    def set_decoder_input(self, probs):
        """Measurement / test hook (scrappie_hip_set_decoder_input): `probs` = list of (T, NS) float32
        probability matrices (reference state order); read i of every later launch group is decoded
        from probs[i % len(probs)] instead of the network's own posterior.  None switches it off."""
        if getattr(self, "_alt_dev", None):
            lib().scrappie_hip_set_decoder_input(self._h, None, None, 0)
            self.free(self._alt_dev)
            self._alt_dev = None
        if probs is None:
            return
        mats = [np.ascontiguousarray(p, dtype=ftype) for p in probs]
        off = np.zeros(len(mats), dtype=np.uint64)
        tot = 0
        for i, m in enumerate(mats):
            off[i] = tot
            tot += m.size
        self._alt_dev = self.upload(np.concatenate([m.ravel() for m in mats]))
        if lib().scrappie_hip_set_decoder_input(self._h, self._alt_dev, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(mats)) != 0:
            raise RuntimeError("set_decoder_input: " + last_error())

    def set_trunk_input(self, trunks):
        """Measurement / test hook (scrappie_hip_set_trunk_input): `trunks` = list of (T, S) float32 activation
        matrices; in every later launch group the output layer of read i reads trunks[i % len(trunks)] instead of
        the trunk's own output, so the default decode path (S1 inside the decoder) sees the posteriors those
        activations encode.  None switches it off."""
        if getattr(self, "_trk_dev", None):
            lib().scrappie_hip_set_trunk_input(self._h, None, None, 0)
            self.free(self._trk_dev)
            self._trk_dev = None
        if trunks is None:
            return
        mats = [np.ascontiguousarray(t, dtype=ftype) for t in trunks]
        off = np.zeros(len(mats), dtype=np.uint64)
        tot = 0
        for i, m in enumerate(mats):
            off[i] = tot
            tot += m.size
        self._trk_dev = self.upload(np.concatenate([m.ravel() for m in mats]))
        if lib().scrappie_hip_set_trunk_input(self._h, self._trk_dev, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(mats)) != 0:
            raise RuntimeError("set_trunk_input: " + last_error())

    def debug_option(self, name, value):
        if lib().scrappie_hip_debug_option(self._h, name.encode(), int(value)) != 0:
            raise RuntimeError("debug_option: " + last_error())

    def debug_fetch(self, what, dtype=np.uint8):
        """A device buffer of the most recent transducer launch group (scrappie_hip_debug_fetch) as a flat array."""
        n = lib().scrappie_hip_debug_fetch(self._h, what.encode(), None, 0)
        if n < 0:
            raise RuntimeError("debug_fetch: " + last_error())
        buf = np.zeros(n, dtype=np.uint8)
        if n and lib().scrappie_hip_debug_fetch(self._h, what.encode(), buf.ctypes.data, n) < 0:
            raise RuntimeError("debug_fetch: " + last_error())
        return buf.view(dtype)

    def debug_split(self, x):
        """The two fp16 pieces of every value of x as the kernels cut them (scrappie_hip_debug_split): (p1, p2), uint16 bit patterns."""
        x = np.ascontiguousarray(x, dtype=ftype).ravel()
        p1, p2 = np.zeros(x.size, np.uint16), np.zeros(x.size, np.uint16)
        fn = lib().scrappie_hip_debug_split
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        if fn(self._h, x.ctypes.data, x.size, p1.ctypes.data, p2.ctypes.data) != 0:
            raise RuntimeError("debug_split: " + last_error())
        return p1, p2

    GATE_FORMS = ("d_logistic", "d_tanh", "d_logistic4", "d_tanh4", "d_logistic4_acc", "d_tanh4_acc", "d_exp", "d_exp_acc",
                  "d_exp_acc_inrange", "d_elu")        # scrappie_hip.h: SH_GATE_*

    def debug_gates(self, which, x):
        """One activation form of the kernels (a name of GATE_FORMS) on every value of x, as float32 (scrappie_hip_debug_gates).
        The *_acc forms are given 2^14 x, formed here in float32 (exact), as the split products hand it to them."""
        x = np.ascontiguousarray(x, dtype=ftype).ravel()
        if which.endswith("_acc") or which.endswith("_acc_inrange"):
            x = x * ftype(16384.0)
        out = np.zeros(x.size, ftype)
        fn = lib().scrappie_hip_debug_gates
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        if fn(self._h, self.GATE_FORMS.index(which), x.ctypes.data, x.size, out.ctypes.data) != 0:
            raise RuntimeError("debug_gates: " + last_error())
        return out

    def debug_stitch(self, path, side=None, nstate=1025, crf=False):
        """k_stitch on one read given on the host: (bases or None, pos, redo)."""
        path = np.ascontiguousarray(path, dtype=np.int32)
        T = len(path) - 1
        sd = None if side is None else np.ascontiguousarray(side, dtype=ftype)
        buf = C.create_string_buffer(5 * (T + 1) + 16)
        pos = np.zeros(T + 1, np.int32)
        redo = C.c_int(0)
        n = lib().scrappie_hip_debug_stitch(self._h, path.ctypes.data_as(C.POINTER(C.c_int)),
                                            None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_float)), T, nstate, 1 if crf else 0,
                                            buf, len(buf), pos.ctypes.data_as(C.POINTER(C.c_int)), C.byref(redo))
        if n == -2:
            raise RuntimeError("debug_stitch: " + last_error())
        return (buf.value.decode() if n >= 0 else None), pos, redo.value

    def debug_stitch_dwell(self, paths, dwells, prior_num, nstate=1025, cap=None, trailing=0):
        """k_stitch_dwell (the dwell-corrected stitching of the events path) on a batch of reads given on the host, one
        launch: paths[i] has len(dwells[i]) + trailing entries, prior_num[i] is the last event's length + the span of
        the starts, cap[i] the bytes of the device's bases buffer read i owns (default: what the engine reserves).
        Returns (bases, lengths, pos, redo, buffer): the call of each read (None: no call, or left to the host),
        the lengths and flags as the device wrote them, overlapper's pos[] per read, and per read the whole of its
        reservation as the device left it."""
        n = len(paths)
        nent = np.array([len(d) for d in dwells], dtype=np.uintp)
        for pth, d in zip(paths, dwells):
            if len(pth) != len(d) + trailing:
                raise ValueError("a path of len(dwell) + trailing entries")
        cap = np.array([dwell_capacity(len(pth)) for pth in paths] if cap is None else cap, dtype=np.uintp)
        rcap = (cap + 15) // 16 * 16
        boff = np.concatenate(([0], np.cumsum(rcap))).astype(np.int64)
        flat_p = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x in paths]), dtype=np.int32)
        flat_d = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x in dwells]), dtype=np.int32)
        num = np.ascontiguousarray(prior_num, dtype=ftype)
        buf = np.zeros(int(boff[-1]), dtype=np.uint8)
        lengths, redo = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pos = np.zeros(len(flat_p), np.int32)
        ip, sp = C.POINTER(C.c_int), C.POINTER(C.c_size_t)
        if lib().scrappie_hip_debug_stitch_dwell(self._h, flat_p.ctypes.data_as(ip), flat_d.ctypes.data_as(ip), nent.ctypes.data_as(sp), n, trailing,
                                                 num.ctypes.data_as(C.POINTER(C.c_float)), nstate, cap.ctypes.data_as(sp), buf.ctypes.data, len(buf),
                                                 lengths.ctypes.data_as(ip), pos.ctypes.data_as(ip), redo.ctypes.data_as(ip)) != 0:
            raise RuntimeError("debug_stitch_dwell: " + last_error())
        raw = [buf[boff[i]:boff[i + 1]] for i in range(n)]
        bases = [bytes(raw[i][:lengths[i]]).decode() if lengths[i] >= 0 and not redo[i] else None for i in range(n)]
        poff = np.concatenate(([0], np.cumsum([len(x) for x in paths])))
        return bases, lengths, [pos[poff[i]:poff[i + 1]] for i in range(n)], redo, raw

    def posterior(self, signal, model='rgrgr_r94', min_prob=1e-5, tempW=1.0, tempb=1.0, log=True):
        """(T, NS) array, reference state order (stay last)."""
        rt = RawTable(signal)
        m = lib().scrappie_hip_posterior(self._h, self._models[model], rt.data(), min_prob, tempW, tempb, log)
        if not m:
            raise RuntimeError("posterior: " + last_error())
        return ScrappyMatrix(m).data(as_numpy=True, sloika=False)

    def read_blocks(self, model, nsample):
        """posterior columns (blocks) of a read of `nsample` samples; 0 below the model's minimum"""
        return lib().scrappie_hip_read_blocks(self._h, self._models[model], nsample)

    def map_to_sequence(self, signals, sequences, model='rgrgr_r94', viterbi=True, path=False, bands=None, stay_pen=0.0,
                        skip_pen=0.0, local_pen=4.0, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Block-based mapping of each read (trimmed, normalised float32 signal) to its base sequence, batched: the
        network and S1 run as for `posterior`, the posterior stays on the device, only scores and paths return
        (scrappie_hip_map_batch).  `bands`: None, an int (scrappy's diagonal band, per read) or a list with a
        (low, high) pair or None per read.  Returns [(score, path or None)] in input order; score NaN where a read
        cannot be mapped (too short, a bad sequence or band).
        With a flip-flop (CRF) model (`rnnrf_r94`) it is the global alignment of `map_trans_to_sequence` on the read's own
        transitions (k_map_crf): a band holds nblock + 1 entries of cells (an int: `map_crf_diagonal_band`), a path
        nblock + 1 entries, banded reads return one too, and the penalties are not used."""
        n = len(signals)
        if len(sequences) != n:
            raise ValueError("one sequence per signal")
        _path_needs_viterbi(path, viterbi)
        h = self._models[model]
        nstate = lib().scrappie_hip_model_states(self._h, h)
        crf = nstate == 25                  # the flip-flop models: 5 x 5 transitions, bases as codes of one
        kmer_len = 1 if crf else guess_state_properties(nstate)[1]
        rts, keep = _raw_tables(signals)
        tgs = (_MapTarget * n)()
        for i, (x, sq) in enumerate(zip(keep[:n], sequences)):
            try:
                codes = encode_bases(sq, kmer_len)
            except ValueError:
                codes = np.zeros(0, dtype=np.int32)      # mapped to NaN by the library (empty sequence)
            keep.append(codes)
            tgs[i].seq = codes.ctypes.data_as(C.POINTER(C.c_int))
            tgs[i].seqlen = len(codes)
            b = bands if (bands is None or isinstance(bands, int)) else bands[i]
            if isinstance(b, int):
                nblock = self.read_blocks(model, len(x))
                if nblock <= 0 or len(codes) == 0:
                    b = None
                else:
                    b = map_crf_diagonal_band(nblock, len(codes), b) if crf else diagonal_bands(b, nblock, len(codes))
            if b is not None:
                lo, hi = (np.ascontiguousarray(v, dtype=np.uintp) for v in b)
                keep += [lo, hi]
                tgs[i].poslow = lo.ctypes.data_as(C.POINTER(C.c_size_t))
                tgs[i].poshigh = hi.ctypes.data_as(C.POINTER(C.c_size_t))
        p = self.default_params(min_prob=min_prob, tempW=tempW, tempb=tempb, stay_pen=stay_pen, skip_pen=skip_pen,
                                local_pen=local_pen)
        out = (_MapResult * n)()
        if lib().scrappie_hip_map_batch(self._h, h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError("map_batch: " + last_error())
        res = _scores_and_paths(out, n, 'nblock', 1 if crf else 0)
        lib().scrappie_hip_free_map_results(out, n)
        return res

    def map_to_sequences(self, signals, candidates, model='rgrgr_r94', viterbi=True, path=False, stay_pen=0.0, skip_pen=0.0,
                         local_pen=4.0, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Which of these sequences is this read?  Each read (trimmed, normalised float32 signal) against every one of its
        candidate base sequences, unbanded: the network and S1 run once per read, the candidates are packed into workgroups
        of k_map_pack on the resident posterior (scrappie_hip_map_multi_batch).  `candidates`: a list of base strings shared
        by every read (encoded once), or one list of strings per read.  Returns [(scores, best, path or None)] in input
        order: the float32 raw scores as `map_to_sequence` gives them (NaN where a candidate, or the read, cannot be
        mapped; normalising for length is the caller's business), the index of the highest (the lowest index on a tie,
        -1: none) and, with `path`, the Viterbi path of that candidate."""
        def targets():
            nstate = lib().scrappie_hip_model_states(self._h, self._models[model])
            if nstate == 25:
                raise RuntimeError("map_multi_batch: a flip-flop (CRF) model maps one sequence per read (map_to_sequence)")
            kmer_len = guess_state_properties(nstate)[1]
            return lambda cl: _map_targets(cl, kmer_len)
        return Engine._map_multi(self, "map_multi_batch", lib().scrappie_hip_map_multi_batch, signals, candidates, model, targets,
                                 dict(min_prob=min_prob, tempW=tempW, tempb=tempb, stay_pen=stay_pen, skip_pen=skip_pen, local_pen=local_pen),
                                 viterbi, path, 0)

    def _map_multi(self, fn_name, symbol, signals, candidates, model, targets, params, viterbi, path, more):
        """A *_multi_batch symbol on the reads and their candidates.  The argument checks come before anything touches the engine:
        `targets()` gives how a list of candidates becomes map targets, `params` are `default_params`' keywords; `more`: the
        entries a path has beyond the read's blocks."""
        n = len(signals)
        _path_needs_viterbi(path, viterbi)
        candidates, shared = _per_read_lists(candidates, n, 'candidates')
        h = self._models[model]
        encode = targets()
        rts, keep = _raw_tables(signals)
        cds, kept = _per_read_sets(candidates, shared, n, encode)
        keep += kept
        p = self.default_params(**params)
        out = (_MapMultiResult * max(n, 1))()
        if symbol(self._h, h, rts, cds, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError(fn_name + ": " + last_error())
        res = []
        rs = [out[i] for i in range(n)]
        for r, pth in zip(rs, _paths(rs, more=more)):
            sc = np.ctypeslib.as_array(r.score, shape=(r.ncand,)).copy() if r.ncand else np.zeros(0, dtype=np.float32)
            res.append((sc, int(r.best), pth))
        lib().scrappie_hip_free_map_multi_results(out, n)
        return res

    def map_to_sequences_crf(self, signals, candidates, model='rnnrf_r94', viterbi=True, path=False, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Which of these sequences is this read, under a flip-flop (CRF) model?  Each read (trimmed, normalised float32 signal)
        against every one of its candidate base sequences, unbanded: the network and k_crf run once per read, the candidates
        are packed into workgroups of k_map_crf_pack on the resident transitions (scrappie_hip_map_crf_multi_batch).
        `candidates`: a list of base strings shared by every read (encoded once), or one list of strings per read.  Returns
        [(scores, best, path or None)] in input order: the float32 scores as `map_to_sequence(model='rnnrf_r94')` gives them
        (NaN where a candidate, or the read, cannot be mapped), the index of the highest (the lowest index on a tie, -1:
        none) and, with `path`, the Viterbi path of that candidate, nblock + 1 entries."""
        return Engine._map_multi(self, "map_crf_multi_batch", lib().scrappie_hip_map_crf_multi_batch, signals, candidates, model,
                                 lambda: _crf_targets, dict(min_prob=min_prob, tempW=tempW, tempb=tempb), viterbi, path, 1)

    def map_to_reference(self, signals, references, model='rnnrf_r94', viterbi=True, path=False, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Where in its reference does each read lie?  Each read (trimmed, normalised float32 signal) of a flip-flop (CRF)
        model mapped INTO a longer base sequence, batched (scrappie_hip_map_local_batch): the network runs as for
        `posterior`, the transitions stay on the device, every window of every reference is one workgroup of
        k_map_crf_local.  `references`: one string for all reads (encoded and uploaded once), or one per read.  Returns
        [(score, first, last, path)] in input order as `map_trans_to_reference` gives them; score NaN (and None) where a
        read or its reference cannot be mapped."""
        n = len(signals)
        _path_needs_viterbi(path, viterbi)
        tgs, enc = _reference_targets(_per_read_references(references, n), 1)
        h = self._models[model]
        rts, keep = _raw_tables(signals)
        keep.append(enc)
        p = self.default_params(min_prob=min_prob, tempW=tempW, tempb=tempb)
        out = (_MapLocalResult * max(n, 1))()
        if lib().scrappie_hip_map_local_batch(self._h, h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError("map_local_batch: " + last_error())
        res = _located(out, n, viterbi, more=1)
        lib().scrappie_hip_free_map_local_results(out, n)
        return res

    def map_to_reference_transducer(self, signals, references, model='rgrgr_r94', viterbi=True, path=False, stay_pen=0.0, skip_pen=0.0,
                                    local_pen=4.0, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Where in its reference does each read lie?  Each read (trimmed, normalised float32 signal) of a transducer model
        mapped INTO a longer base sequence, batched (scrappie_hip_map_post_local_batch): the network and S1 run as for
        `posterior`, the posterior stays on the device, every window of every reference is one workgroup of k_map_local.
        `references`: one string for all reads (encoded with `encode_bases(ref, kmer_len)` and uploaded once), or one per
        read.  Returns [(score, first, last, path)] in input order as `map_post_to_reference` gives them; score NaN (and
        None) where a read or its reference cannot be mapped."""
        n = len(signals)
        _path_needs_viterbi(path, viterbi)
        references = _per_read_references(references, n)
        h = self._models[model]
        nstate = lib().scrappie_hip_model_states(self._h, h)
        kmer_len = 1 if nstate == 25 else guess_state_properties(nstate)[1]      # (a flip-flop model: refused by the library)
        tgs, enc = _reference_targets(references, kmer_len)
        rts, keep = _raw_tables(signals)
        keep.append(enc)
        p = self.default_params(min_prob=min_prob, tempW=tempW, tempb=tempb, stay_pen=stay_pen, skip_pen=skip_pen, local_pen=local_pen)
        out = (_MapLocalResult * max(n, 1))()
        if lib().scrappie_hip_map_post_local_batch(self._h, h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError("map_post_local_batch: " + last_error())
        res = _located(out, n, viterbi)
        lib().scrappie_hip_free_map_local_results(out, n)
        return res

    def find_sequences(self, signals, motifs, model='rnnrf_r94', positions=True, min_prob=1e-5, tempW=1.0, tempb=1.0):
        """Which of these short sequences occur inside each read, and where?  Each read (trimmed, normalised float32 signal) of a
        flip-flop (CRF) model searched for every one of its motifs, batched (scrappie_hip_find_batch): the network runs as for
        `posterior`, the transitions stay on the device, all motifs of all reads of a launch group are packed into the
        workgroups of one k_crf_find launch.  `motifs`: one list of base strings for all reads (encoded and uploaded once), or
        one list per read.  Returns [(scores, call_score, best, begins, ends)] in input order, as `find_in_trans` gives them;
        best: the index of the highest finite score (the lowest on a tie, -1: none).  A read that cannot run has every score
        NaN and best -1.  begins and ends are entries of the path, 0 .. nblock: entry t lies at sample t * stride of the read
        (stride: the model's convolution stride; `read_blocks` gives nblock), so the motif covers samples
        [begin * stride, (end + 1) * stride).  A
        motif is searched as given: pass its reverse complement as another motif for the other strand."""
        n = len(signals)
        motifs, shared = _per_read_lists(motifs, n, 'motifs')
        h = self._models[model]
        rts, keep = _raw_tables(signals)
        cds, kept = _per_read_sets(motifs, shared, n, lambda ml: _motif_targets(ml, False))
        keep += kept
        p = self.default_params(min_prob=min_prob, tempW=tempW, tempb=tempb)
        out = (_FindResult * max(n, 1))()
        if lib().scrappie_hip_find_batch(self._h, h, rts, cds, n, C.byref(p), 1 if positions else 0, out) != 0:
            raise RuntimeError("find_batch: " + last_error())
        res = []
        for r in (out[i] for i in range(n)):
            k = int(r.nmotif)
            take = lambda q, dt: (np.ctypeslib.as_array(q, shape=(k,)).copy() if k else np.zeros(0, dtype=dt))
            res.append((take(r.score, np.float32), np.float32(r.call_score), int(r.best),
                        take(r.begin, np.int32) if positions else None, take(r.end, np.int32) if positions else None))
        lib().scrappie_hip_free_find_results(out, n)
        return res

    @staticmethod
    def _bands_per_read(bands, n):
        """`bands` of score_edits as a list of None, an int or a (low, high) pair per read"""
        if isinstance(bands, (int, np.integer)):
            return [int(bands)] * n
        bands = list(bands)
        # an edge of a band: a sequence of numbers (a per-read entry is None, an int, or a pair of such sequences); decided from the
        # first element alone, so that a ragged pair never reaches numpy
        one = lambda b: b is not None and not isinstance(b, (int, np.integer)) and len(b) > 0 and isinstance(b[0], (int, float, np.number))
        if len(bands) == 2 and one(bands[0]) and one(bands[1]):             # one (low, high) pair for all reads
            return [bands] * n
        if len(bands) != n:
            raise ValueError("`bands`: None, an int, a (low, high) pair, or one of these per signal")
        return bands

    def score_edits(self, signals, sequences, model='rnnrf_r94', viterbi=False, min_prob=1e-5, tempW=1.0, tempb=1.0, bands=None):
        """Is any single-base edit of this sequence better than the sequence?  Each read (trimmed, normalised float32 signal)
        of a flip-flop (CRF) model against EVERY single-base edit of its sequence, batched (scrappie_hip_map_crf_edits_batch):
        the network and k_crf run once per read; a forward sweep, a backward sweep and one combining pass score all 9 L + 4
        edits.  `sequences`: one base string (or array of base codes) for all reads -- a window of a draft that the reads
        cover --, or one per read.  Returns [(base, sub, dele, ins)] in input order as `map_trans_edits` gives them; with
        `viterbi=False` the scores are log-likelihoods, so `sum(r[1] - r[0] for r in res)` over the reads of a window is the
        log-likelihood ratio of every substitution.  A read or a sequence that cannot be scored has everything NaN
        (`last_error()` names the first).
        `bands`: None (exactly the call above), an int (the diagonal band of that half-width per read, `map_crf_diagonal_band`),
        a (low, high) pair of nblock + 1 entries each for all reads, or a list with None, an int or such a pair per read --
        `map_crf_path_band(path, len(seq), halfwidth)` on the paths of `map_to_sequence(..., path=True)` makes them.  The edits
        are then scored inside the bands (scrappie_hip_map_crf_edits_banded_batch): rows, traffic and time go with the cells in
        the band; a read with None takes the unbanded kernels; a band that is not valid for its read (or not of nblock + 1
        entries) leaves that read NaN."""
        if bands is None:
            return _score_edits(self, lib().scrappie_hip_map_crf_edits_batch, "map_crf_edits_batch", signals, sequences, model, viterbi,
                                     min_prob=min_prob, tempW=tempW, tempb=tempb)
        return _score_edits(self, lib().scrappie_hip_map_crf_edits_banded_batch, "map_crf_edits_banded_batch", signals, sequences, model, viterbi,
                            bands=Engine._bands_per_read(bands, len(signals)), min_prob=min_prob, tempW=tempW, tempb=tempb)

    def score_edits_transducer(self, signals, sequences, model='rgrgr_r94', viterbi=False, stay_pen=0.0, skip_pen=0.0, local_pen=4.0,
                               min_prob=1e-5, tempW=1.0, tempb=1.0, bands=None):
        """`score_edits` for the transducer models (scrappie_hip_map_edits_batch; k_map_edits_rows, k_map_edits): each read
        against EVERY single-base edit of its sequence under `map_to_sequence`'s lattice with these penalties -- an edit of one
        base changes up to k consecutive k-mer states.  The network and S1 run once per read.  `sequences`: one base string (or
        array of base codes) for all reads, or one per read.  Returns [(base, sub, dele, ins)] in input order as
        `map_post_edits` gives them, numbered by `apply_edit`; base is `map_to_sequence`'s score of the sequence itself.  A
        read or a sequence that cannot be scored has everything NaN (`last_error()` names the first).
        `bands`: None (exactly the call above), an int (scrappy's `diagonal_bands` for the read's block count and the n = L - k + 1
        states), a (low, high) pair of nblock entries each for all reads, or a list with None, an int or such a pair per read --
        `map_path_band(path, n, halfwidth)` on the paths of `map_to_sequence(..., path=True)` makes them.  The edits are then
        scored inside the bands (scrappie_hip_map_edits_banded_batch): rows, traffic and time go with the cells in the band; a read
        with None takes the unbanded kernels; a band that is not valid for its read (or not of nblock entries) leaves that read
        NaN.  base is then the masked programme's score, not `map_to_sequence(..., bands=...)`'s."""
        pen = dict(min_prob=min_prob, tempW=tempW, tempb=tempb, stay_pen=stay_pen, skip_pen=skip_pen, local_pen=local_pen)
        if bands is None:
            return _score_edits(self, lib().scrappie_hip_map_edits_batch, "map_edits_batch", signals, sequences, model, viterbi, **pen)
        return _score_edits(self, lib().scrappie_hip_map_edits_banded_batch, "map_edits_banded_batch", signals, sequences, model, viterbi,
                            bands=Engine._bands_per_read(bands, len(signals)), kmer_len=-1, **pen)

    def _edits_timing(self, fn):
        t = (C.c_double * 3)()
        nl, nb = C.c_size_t(0), C.c_size_t(0)
        fn(self._h, t, C.byref(nl), C.byref(nb))
        return dict(rows_forward_ms=t[0], rows_backward_ms=t[1], edits_ms=t[2], launches=int(nl.value), row_bytes=int(nb.value))

    def crf_edits_timing(self):
        """the last score_edits call: device ms of the forward rows, the backward rows and the combining pass, summed over its
        launches; how many launches of the three it made and their row bytes"""
        return self._edits_timing(lib().scrappie_hip_crf_edits_timing)

    def map_edits_timing(self):
        """the same for the last score_edits_transducer call"""
        return self._edits_timing(lib().scrappie_hip_map_edits_timing)

    def _timing(self, fn, names):
        t = (C.c_double * 3)()
        fn(self._h, t)
        return dict(zip(names, t))

    def map_timing(self):
        """the last map_to_sequence call's time (ms, summed over launch groups): network + S1, k_map, walk + results"""
        return self._timing(lib().scrappie_hip_map_timing, ('network_ms', 'map_ms', 'walk_ms'))

    def match_squiggle(self, signals, squiggles, viterbi=True, path=False, rate=1.0, back_prob=0.0, local_pen=2.0,
                       skip_pen=5000.0, min_score=5.0, band=None):
        """Each signal (trimmed, normalised float32 array, or a `RawTable` with its window) against its predicted squiggle
        (an (npos, 3) array of mean, log sd, dwell logit), batched (scrappie_hip_squiggle_match_batch).  Returns
        [(score, path or None)] in input order; score NaN where a read cannot be mapped.  `band`: None, an int (diagonal
        half-width in positions) or a (low, width) pair for all reads, or a list with one of these per read
        (scrappie_hip_squiggle_match_banded_batch); score NaN too where a band is invalid or admits no path."""
        n = len(signals)
        if len(squiggles) != n:
            raise ValueError("one squiggle per signal")
        _path_needs_viterbi(path, viterbi)
        rts, keep = _raw_tables(signals)
        tgs = (_SquigTarget * n)()
        for i, sq in enumerate(squiggles):
            if isinstance(sq, str):
                _squiggle_matrix(sq)
            sq = np.ascontiguousarray(sq, dtype=ftype)
            if sq.ndim != 2 or sq.shape[1] < 3:
                raise ValueError("a squiggle should be an (npos, 3) array")
            keep.append(sq)
            tgs[i] = _SquigTarget(sq.ctypes.data_as(C.POINTER(C.c_float)), sq.shape[0], sq.shape[1])
        p = _SquigParams(rate, back_prob, local_pen, skip_pen, min_score)
        out = (_SquigResult * n)()
        if band is None:
            rc = lib().scrappie_hip_squiggle_match_batch(self._h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out)
        else:
            if isinstance(band, list) and len(band) != n:
                raise ValueError("one band per signal")
            bds = (_SquigBand * max(n, 1))()
            for i in range(n):
                low, width = _squiggle_band(band[i] if isinstance(band, list) else band,
                                            max(int(rts[i].end) - int(rts[i].start), 0), int(tgs[i].npos))
                keep.append(low)
                bds[i] = _SquigBand(low.ctypes.data_as(C.POINTER(C.c_int32)) if low is not None else None, width)
            rc = lib().scrappie_hip_squiggle_match_banded_batch(self._h, rts, tgs, bds, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out)
        if rc != 0:
            raise RuntimeError("squiggle_match_batch: " + last_error())
        res = _scores_and_paths(out, n, 'n')
        lib().scrappie_hip_free_squiggle_results(out, n)
        return res

    def match_squiggle_reference(self, signals, references, viterbi=True, path=False, rate=1.0, back_prob=0.0, local_pen=2.0,
                                 skip_pen=5000.0, min_score=5.0):
        """Where inside a longer reference squiggle does each signal lie?  Each signal (trimmed, normalised float32 array, or a
        `RawTable` with its window) INTO its reference (an (npos, 3) array), batched (scrappie_hip_squiggle_match_local_batch; every
        window of every read a workgroup of k_squig_local).  `references`: one array for all reads -- turned into tables once per
        call and uploaded once per launch --, or a list with one per read (the same array object given twice counts once).
        Returns [(score, first, last, path)] in input order as `squiggle_match_reference` gives them; score NaN where a read
        cannot be mapped."""
        n = len(signals)
        _path_needs_viterbi(path, viterbi)
        if isinstance(references, np.ndarray) and references.ndim == 2:
            references = [references] * n
        references = list(references)
        if len(references) != n:
            raise ValueError("one reference for all signals, or one per signal")
        rts, keep = _raw_tables(signals)
        tgs = (_SquigTarget * max(n, 1))()
        made = {}
        for i, sq in enumerate(references):
            if id(sq) not in made:
                a = np.ascontiguousarray(sq, dtype=ftype)
                if a.ndim != 2 or a.shape[1] < 3:
                    raise ValueError("a reference should be an (npos, 3) array")
                made[id(sq)] = a
            a = made[id(sq)]
            tgs[i] = _SquigTarget(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], a.shape[1])
        keep.append(made)
        p = _SquigParams(rate, back_prob, local_pen, skip_pen, min_score)
        out = (_SquigLocalResult * max(n, 1))()
        if lib().scrappie_hip_squiggle_match_local_batch(self._h, rts, tgs, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError("squiggle_match_local_batch: " + last_error())
        res = _located(out, n, viterbi, 'n')
        lib().scrappie_hip_free_squiggle_local_results(out, n)
        return res

    def mappy_reference(self, signals, sequences, model='squiggle_r94', rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0,
                        min_score=5.0):
        """Each signal INTO the squiggle predicted for a longer base sequence: one batched prediction over the DISTINCT
        sequences, then `match_squiggle_reference` with paths.  `sequences`: one string for all reads or one per read.  Returns
        [(score, first, last, path)]; (nan, None, None, None) where a sequence or a read is refused."""
        n = len(signals)
        if isinstance(sequences, str):
            sequences = [sequences] * n
        sequences = list(sequences)
        if len(sequences) != n:
            raise ValueError("one sequence for all signals, or one per signal")
        distinct = sorted(set(sequences))
        sq = dict(zip(distinct, self.predict_squiggle(distinct, model=model, rescale=False))) if distinct else {}
        keep = [i for i in range(n) if sq[sequences[i]] is not None]
        got = self.match_squiggle_reference([signals[i] for i in keep], [sq[sequences[i]] for i in keep], viterbi=True, path=True, rate=rate,
                                            back_prob=back_prob, local_pen=local_pen, skip_pen=skip_pen, min_score=min_score)
        res = [(float("nan"), None, None, None)] * n
        for i, r in zip(keep, got):
            res[i] = r
        return res

    def match_squiggles(self, signals, candidates, viterbi=True, path=False, rate=1.0, back_prob=0.0, local_pen=2.0,
                        skip_pen=5000.0, min_score=5.0):
        """Which of these squiggles does this signal fit best?  Each signal (trimmed, normalised float32 array, or a
        `RawTable` with its window) against every one of its candidate squiggles ((npos, 3) arrays), unbanded: the signal
        is uploaded once and the candidates are packed into workgroups of k_squig_pack
        (scrappie_hip_squiggle_match_multi_batch).  `candidates`: one list of arrays shared by every read (turned into
        tables and uploaded once per launch), or one list of arrays per read.  Returns [(scores, best, path or None)] in
        input order: the float32 raw scores as `match_squiggle` gives them (NaN where a candidate, or the read, cannot be
        matched), the index of the highest (the lowest index on a tie, -1: none) and, with `path`, the Viterbi path of
        that candidate over the whole signal."""
        n = len(signals)
        _path_needs_viterbi(path, viterbi)
        candidates = list(candidates)
        shared = all(isinstance(c, np.ndarray) and c.ndim == 2 for c in candidates)
        if not shared and len(candidates) != n:
            raise ValueError("one list of candidates per signal")
        rts, keep = _raw_tables(signals)
        cds = (_SquigCandidates * max(n, 1))()
        if shared:
            made = [_squig_targets(candidates)]
            for i in range(n):
                cds[i].cand, cds[i].ncand = made[0][0], len(candidates)
        else:
            made = []
            for i, c in enumerate(candidates):
                c = list(c)
                made.append(_squig_targets(c))
                cds[i].cand, cds[i].ncand = made[i][0], len(c)
        keep += made
        p = _SquigParams(rate, back_prob, local_pen, skip_pen, min_score)
        out = (_SquigMultiResult * max(n, 1))()
        if lib().scrappie_hip_squiggle_match_multi_batch(self._h, rts, cds, n, C.byref(p), 1 if viterbi else 0, 1 if path else 0, out) != 0:
            raise RuntimeError("squiggle_match_multi_batch: " + last_error())
        res = []
        rs = [out[i] for i in range(n)]
        for r, pth in zip(rs, _paths(rs, 'n')):
            sc = np.ctypeslib.as_array(r.score, shape=(r.ncand,)).copy() if r.ncand else np.zeros(0, dtype=np.float32)
            res.append((sc, int(r.best), pth))
        lib().scrappie_hip_free_squiggle_multi_results(out, n)
        return res

    def mappy_multi(self, signals, sequences, model='squiggle_r94', rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0,
                    min_score=5.0):
        """Each signal against the squiggles predicted for its candidate base sequences: one batched prediction over the
        DISTINCT sequences, then `match_squiggles` with paths.  `sequences`: one list of strings shared by every read, or
        one list per read.  Returns [(scores, best, path or None)]; a sequence that is refused scores NaN."""
        n = len(signals)
        seqs, shared = _per_read_lists(sequences, n, 'sequences')
        distinct = sorted(set(seqs) if shared else set(s for lst in seqs for s in lst))
        sq = dict(zip(distinct, self.predict_squiggle(distinct, model=model, rescale=False))) if distinct else {}
        empty = np.zeros((0, 3), dtype=ftype)
        take = lambda lst: [sq[s] if sq[s] is not None else empty for s in lst]
        cands = take(seqs) if shared else [take(list(lst)) for lst in seqs]
        return self.match_squiggles(signals, cands, viterbi=True, path=True, rate=rate, back_prob=back_prob, local_pen=local_pen,
                                    skip_pen=skip_pen, min_score=min_score)

    def predict_squiggle(self, sequences, model='squiggle_r94', rescale=False):
        """The predicted squiggle of each base sequence (a str over ACGT, or an int array of codes 0..3), batched
        (scrappie_hip_squiggle_predict_batch): a list of (npos, 3) float32 arrays of (mean, log sd, dwell logit) -- with
        rescale (mean, sd, expected dwell) -- in input order, None where a sequence is refused (`last_error()` says why).
        `model`: a squiggle model loaded on this engine."""
        n = len(sequences)
        ip = C.POINTER(C.c_int)
        codes = [_base_codes(x) if isinstance(x, str) else np.ascontiguousarray(x, dtype=np.int32) for x in sequences]
        ptrs = (ip * max(n, 1))(*[c.ctypes.data_as(ip) for c in codes])
        lens = (C.c_size_t * max(n, 1))(*[len(c) for c in codes])
        out = (C.POINTER(_Mat) * max(n, 1))()
        if lib().scrappie_hip_squiggle_predict_batch(self._h, model.encode(), ptrs, lens, n, 1 if rescale else 0, out) != 0:
            raise RuntimeError("squiggle_predict_batch: " + last_error())
        res = []
        for i in range(n):
            res.append(ScrappyMatrix(out[i]).data(as_numpy=True, sloika=False) if out[i] else None)
        return res

    def sqnet_timing(self):
        """the last predict_squiggle call's time (ms, summed over launches): upload, k_sqnet, download + transform"""
        return self._timing(lib().scrappie_hip_sqnet_timing, ('upload_ms', 'net_ms', 'download_ms'))

    def mappy(self, signals, sequences, model='squiggle_r94', rate=1.0, back_prob=0.0, local_pen=2.0, skip_pen=5000.0,
              min_score=5.0, band=None):
        """Each signal (trimmed, normalised float32 array, or a `RawTable` with its window) against the squiggle predicted
        for its base sequence: one batched prediction, then one batched Viterbi match of the downloaded squiggles.
        Returns [(score, path)] in input order; (nan, None) where a sequence or a read is refused.  `band`: as
        `match_squiggle` takes it (`scrappie mappy --band N` is band=N)."""
        if len(signals) != len(sequences):
            raise ValueError("one sequence per signal")
        sqs = self.predict_squiggle(sequences, model=model, rescale=False)
        keep = [i for i, sq in enumerate(sqs) if sq is not None]
        if isinstance(band, list):
            if len(band) != len(signals):
                raise ValueError("one band per signal")
            band = [band[i] for i in keep]
        got = self.match_squiggle([signals[i] for i in keep], [sqs[i] for i in keep], viterbi=True, path=True, rate=rate,
                                  back_prob=back_prob, local_pen=local_pen, skip_pen=skip_pen, min_score=min_score, band=band)
        res = [(float("nan"), None)] * len(signals)
        for i, r in zip(keep, got):
            res[i] = r
        return res

    def squiggle_timing(self):
        """the last match_squiggle call's time (ms, summed over launches): tables + uploads, k_squig, walk + results"""
        return self._timing(lib().scrappie_hip_squiggle_timing, ('tables_ms', 'match_ms', 'walk_ms'))

    def detect_events(self, signals, window_length1=3, window_length2=6, threshold1=1.4, threshold2=9.0, peak_height=0.2):
        """detect_events for each signal (pA; a float32 array, or a `RawTable` with its window), batched
        (scrappie_hip_detect_events_batch): a list of structured arrays with the event_t layout
        (scrappie_amd.synth.EVENT_DTYPE) in input order, None where a read has no peak or is refused."""
        n = len(signals)
        rts, keep = _raw_tables(signals)
        p = DetectorParam(window_length1, window_length2, threshold1, threshold2, peak_height)
        out = (_EventResult * max(n, 1))()
        if lib().scrappie_hip_detect_events_batch(self._h, rts, n, C.byref(p), out) != 0:
            raise RuntimeError("detect_events_batch: " + last_error())
        return [_take_events(out[i].events) for i in range(n)]

    def event_timing(self):
        """the last detect_events call's time (ms, summed over launches): staging + upload, the kernels, tables to the host"""
        return self._timing(lib().scrappie_hip_event_timing, ('upload_ms', 'detect_ms', 'download_ms'))

    def basecall_events(self, signals, model='nanonet_events', detector=None, dwell=False, **params):
        """Basecall from events, as `scrappie events` does (scrappie_events.c:278-321): detect_events (batched) -> event_features
        -> the events model's posterior -> decode_transducer -> overlapper, the last three as one `basecall` of the feature
        matrices with the homopolymer pass off -- and, with `dwell`, its dwell correction of homopolymer lengths, the whole as one
        scrappie_hip_basecall_events_batch with the stitching in dwell mode.  `signals`: pA, windows already trimmed;
        `detector`: a dict of detect_events' parameters; `params`: fields of `Params` (min_prob, skip_pen, ...).  Returns
        the list `basecall` returns, None where a read has no events or no call."""
        if dwell:
            n = len(signals)
            rts, keep = _raw_tables(signals)
            dp = DetectorParam(**(detector or {}))
            kw = dict(homopolymer=0)
            kw.update(params)
            p = self.default_params(**kw)
            calls = (_Call * max(n, 1))()
            if lib().scrappie_hip_basecall_events_batch(self._h, self._models[model], rts, n, C.byref(dp), C.byref(p), 1, calls) != 0:
                raise RuntimeError("basecall_events_batch: " + last_error())
            return self._unpack(calls, n, p.want_pos)
        evs = self.detect_events(signals, **(detector or {}))
        keep = [i for i, ev in enumerate(evs) if ev is not None]
        kw = dict(homopolymer=0)
        kw.update(params)
        calls = self.basecall([event_features(evs[i]).ravel() for i in keep], model, self.default_params(**kw))
        res = [None] * len(signals)
        for i, c in zip(keep, calls):
            res[i] = c
        return res

    def trunk(self, signal, model='rgrgr_r94', upto=5):
        rt = RawTable(signal)
        m = lib().scrappie_hip_trunk(self._h, self._models[model], rt.data(), upto)
        if not m:
            raise RuntimeError("trunk: " + last_error())
        return ScrappyMatrix(m).data(as_numpy=True, sloika=False)
