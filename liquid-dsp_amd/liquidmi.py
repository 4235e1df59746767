"""ctypes mirror of the liquid_mi355x C-ABI (include/liquid_mi355x.h).

This is the host-side Python view of the drop-in library used by the test
suite and bench.py.  Object names, argument meaning and error behaviour follow
liquid-dsp's liquid.h (firfilt_crcf_create / _execute_block / _destroy ...);
the library itself is C + HIP and runs every sample on the GPU.  Loading the
library never touches the GPU; the first object constructor does, and exits
with a message if no HIP device exists (no CPU fallback).

When torch is imported in the same process, import it BEFORE this module so
that the library binds torch's HIP runtime (one runtime per process).
"""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# LQ_LIB_PATH: an alternative build of the same library (dev/ab/ab.sh A/B runs)
LIB_PATH = os.environ.get("LQ_LIB_PATH") or os.path.join(HERE, "lib", "libliquid_mi355x.so")
HEADER = os.path.join(ROOT, "include", "liquid_mi355x.h")

LIQUID_ANALYZER, LIQUID_SYNTHESIZER = 0, 1
RRRF, CRCF, CCCF = "rrrf", "crcf", "cccf"

_lib = None


class cfloat(C.Structure):
    """liquid_float_complex passed by value (two packed floats)."""
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


def build():
    subprocess.check_call(["make", "-s", "-j8", "-C", HERE])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def set_small_calls(host):
    """Small-call mode (include/liquid_mi355x.h): True computes single-sample
    calls on the host (host/lq_small.c), False (the default) on the GPU."""
    lib().liquid_mi355x_set_small_calls(1 if host else 0)


def get_small_calls():
    return bool(lib().liquid_mi355x_get_small_calls())


def set_max_workgroups(n):
    """Workgroup limit of the persistent kernels (include/liquid_mi355x.h):
    n > 0 launches at most n workgroups, so each walks many tiles; 0 (the
    default) removes the limit.  For tests."""
    lib().liquid_mi355x_set_max_workgroups(int(n))


def get_max_workgroups():
    return int(lib().liquid_mi355x_get_max_workgroups())


PfbRoute = collections.namedtuple("PfbRoute", "route run workgroups chunks")


def channelizer_routes():
    """Every route firpfbch2_route and firpfbch_route can return, by name."""
    L = lib()
    return tuple(L.liquid_mi355x_channelizer_route_name(k).decode()
                 for k in range(L.liquid_mi355x_channelizer_route_count()))


def _pfb_route(fn, args):
    run, wg, ch = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
    r = int(fn(*args, C.byref(run), C.byref(wg), C.byref(ch)))
    if r < 0:
        raise ValueError("%s: bad arguments %r" % (fn.__name__, args))
    return PfbRoute(lib().liquid_mi355x_channelizer_route_name(r).decode(), int(run.value), int(wg.value),
                    int(ch.value))


def firpfbch2_route(typ, M, m, nblocks, parity=0, x_aligned16=True, y_aligned16=True, host_call=False):
    """What a firpfbch2 call of nblocks blocks launches (no GPU call): the
    route's name, the blocks one workgroup run walks, the workgroups and the
    launches (chunks).  liquid_mi355x_firpfbch2_route."""
    return _pfb_route(lib().liquid_mi355x_firpfbch2_route,
                      (int(typ), int(M), int(m), int(nblocks), int(parity) & 1, int(bool(x_aligned16)),
                       int(bool(y_aligned16)), int(bool(host_call))))


def firpfbch_route(t, typ, M, p, nblocks, x_aligned16=True, y_aligned16=True, host_call=False):
    """As firpfbch2_route for firpfbch_crcf / firpfbch_cccf (t "crcf" / "cccf")."""
    return _pfb_route(lib().liquid_mi355x_firpfbch_route,
                      (_KINDS[t], int(typ), int(M), int(p), int(nblocks), int(bool(x_aligned16)),
                       int(bool(y_aligned16)), int(bool(host_call))))


def set_channelizer_chunk(blocks):
    """Blocks per launch of the chunking channelizer analyzers (0: the
    defaults); ValueError where the library refuses the value.  For tests."""
    if lib().liquid_mi355x_set_channelizer_chunk(int(blocks)) != 0:
        raise ValueError("set_channelizer_chunk: %d refused (0, or a multiple of 32 from 64 up)" % blocks)


def get_channelizer_chunk():
    return int(lib().liquid_mi355x_get_channelizer_chunk())


# liquid_mi355x_firdecim_route's codes, by name
FIRDECIM_ROUTES = ("pf_r4x128", "pf_r2x256", "ph2", "pf_r1x256", "ph_r1x64", "plain", "refused")
_KINDS = {"rrrf": 0, "crcf": 1, "cccf": 2}


def firdecim_route(t, M, hlen, aligned16=True, nout=1):
    """The kernel a firdecim device call of nout outputs takes (no GPU call)."""
    return FIRDECIM_ROUTES[lib().liquid_mi355x_firdecim_route(_KINDS[t], M, hlen, 1 if aligned16 else 0, nout)]


def firdecim_tile(route):
    """Outputs per workgroup tile of a route."""
    return int(lib().liquid_mi355x_firdecim_tile(FIRDECIM_ROUTES.index(route)))


def firdecim_grid_cap(t, M, hlen, route):
    """Grid cap of a persistent route at this shape (0: the shape never takes it)."""
    return int(lib().liquid_mi355x_firdecim_grid_cap(_KINDS[t], M, hlen, FIRDECIM_ROUTES.index(route)))


def pinned_input_max():
    """Bytes of input a host-pointer call stages in pinned memory; more goes by DMA."""
    return int(lib().liquid_mi355x_pinned_input_max())


def copyout_max():
    """Bytes of result a host-pointer call returns through the copy-out kernel; more goes by DMA."""
    return int(lib().liquid_mi355x_copyout_max())


def dotprod_block_cap():
    """Grid cap of a dotprod batch launch, in blocks of 256 lanes."""
    return int(lib().liquid_mi355x_dotprod_block_cap())


def dotprod_route(t, n, aligned16=True, nvec=1):
    """(kernel, G, passes) of a dotprod batch call of nvec rows of n samples
    (no GPU call), from the launch's own decision: "vec" (k_dot_vec) or
    "scalar" (k_dot_scalar), the lanes per row, and the passes its grid makes
    over the rows, ceil(nvec G / (256 blocks))."""
    a = (_KINDS[t], n, 1 if aligned16 else 0, nvec)
    r = int(lib().liquid_mi355x_dotprod_route(*a))
    if r < 0:
        raise ValueError("dotprod_route: bad arguments")
    G = 1 << (r & 15)
    lanes = 256 * int(lib().liquid_mi355x_dotprod_blocks(*a))
    return "vec" if r & 16 else "scalar", G, -(-nvec * G // lanes)


def firinterp_route(t, M, L, aligned16=True):
    """The kernel a firinterp / firpfb device call takes for M phases of L
    taps (no GPU call): 0 the plain kernel, else the register-window kernel's
    tap class (8, 12, 16, 20, 24, 32)."""
    return int(lib().liquid_mi355x_firinterp_route(_KINDS[t], M, L, 1 if aligned16 else 0))


def firinterp_max_taps(t):
    """The longest phase, in taps, a firinterp or firpfb object accepts."""
    return int(lib().liquid_mi355x_firinterp_max_taps(_KINDS[t]))


def fftfilt_nfft(t, hlen):
    """Points of fftfilt's segment transform for hlen taps (lqk_fftfilt_nfft):
    4096, 8192, or 0 where the object runs the direct FIR engine instead."""
    fn = lib().lqk_fftfilt_nfft
    fn.restype, fn.argtypes = C.c_uint, [C.c_int, C.c_uint]
    return int(fn(1 if t == RRRF else 0, hlen))


# liquid_mi355x_fft_route's families, by name
FFT_FAMILIES = ("refused", "dft", "k_fft_batch", "fftsmall", "fftr16", "fft1024", "fft4096", "fft8192", "fft16384",
                "four_step", "bluestein", "bluestein_fused")


def fft_route(n, aligned16=True):
    """The kernels an FFT plan of n points takes (no GPU call), by name, from
    the launch's own decision: "dft", "k_fft_batch<8>", "fftsmall<4>",
    "fftr16<2>", "fft1024", "fft4096", "fft8192/a16", "fft8192/a8",
    "four_step 256x128 cols_r<1> rows_s<8>", "bluestein M=64",
    "bluestein_fused M=8192 128x64 cols_s<8> rows_s<4>", "refused"."""
    r = int(lib().liquid_mi355x_fft_route(n, 1 if aligned16 else 0))
    fam = FFT_FAMILIES[r & 15]
    N1, N2, M = 1 << ((r >> 8) & 31), 1 << ((r >> 16) & 31), 1 << ((r >> 24) & 31)
    if fam == "k_fft_batch":
        return "k_fft_batch<%d>" % n
    if fam == "fftsmall":
        return "fftsmall<%d>" % (n // 16)
    if fam == "fftr16":
        return "fftr16<%d>" % (n // 256)
    if fam in ("fft8192", "fft16384"):
        return fam + ("/a16" if r & 16 else "/a8")
    if fam in ("four_step", "bluestein_fused"):
        cols = "cols_r<%d>" % (N1 // 256) if N1 >= 256 else "cols_s<%d>" % (N1 // 16)
        rows = "rows_s<%d>" % (N2 // 16) if r & 32 else "rows_r<%d>" % (N2 // 256)
        return "%s%s %dx%d %s %s" % (fam, " M=%d" % M if fam == "bluestein_fused" else "", N1, N2, cols, rows)
    if fam == "bluestein":
        return "bluestein M=%d" % M
    return fam


def spgram_route(real_in, nfft, W, n=1):
    """The path of a spgram call of n samples (no GPU call): "plain" (gather,
    batch transform, k_spg_part) or the fused kernel's instantiation,
    "fused<float2,HALF,TR>" ..."""
    r = int(lib().liquid_mi355x_spgram_route(1 if real_in else 0, nfft, W, n))
    if r == 0:
        return "plain"
    return "fused<%s,%s,%s>" % ("float" if real_in else "float2", "HALF" if r & 2 else "full", "TR" if r & 4 else "lds")


# liquid_mi355x_iirfilt_route's codes, by name
IIRFILT_ROUTES = ("apply", "scan1", "scan3")


def iirfilt_route(n):
    """The launches of an iirfilt / iirdecim / iirinterp device call of n
    full-rate samples (no GPU call): "apply" (k_iir_apply alone), "scan1" (one
    k_iir_scan launch) or "scan3" (three)."""
    return IIRFILT_ROUTES[lib().liquid_mi355x_iirfilt_route(n)]


def spgram_chunk():
    """Transforms per chunk of spgram's per-bin reduction (SPG_TC)."""
    return int(lib().liquid_mi355x_spgram_chunk())


def spgram_fold_group():
    """Chunks per first-level fold group; more chunks than this fold in two levels."""
    return int(lib().liquid_mi355x_spgram_fold_group())


def spgram_batch_samples():
    """Samples (transforms x nfft) per launch batch of the plain path."""
    return int(lib().liquid_mi355x_spgram_batch_samples())


# liquid_mi355x_resamp_route's and liquid_mi355x_resamp2_route's codes, by name
RESAMP_ROUTES = ("resamp3/const", "resamp3/stride", "resamp/", "generic/", "resamp4/up", "resamp4/up_r4",
                 "resamp4/down", "resamp4/down_dn")
RESAMP2_ROUTES = ("filter", "tiled_b", "tiled")


def resamp_route(t, rate, m, npfb, nx):
    """(kernel/class, tile) of the first block call of nx inputs on a fresh
    resamp object (no GPU call); the tile in inputs (resamp3, resamp,
    generic) or outputs (resamp4).  Reads LQ_RESAMP_INPUT_PLAN as the object does."""
    tile = C.c_uint(0)
    r = lib().liquid_mi355x_resamp_route(_KINDS[t], rate, m, npfb, nx, C.byref(tile))
    if r < 0:
        raise ValueError("resamp_route: bad arguments")
    return RESAMP_ROUTES[r], int(tile.value)


def resamp2_route(mode, m, nbytes):
    """(kernel, calls per tile) of a resamp2 block call reading nbytes of input."""
    tile = C.c_uint(0)
    r = lib().liquid_mi355x_resamp2_route(mode, m, nbytes, C.byref(tile))
    if r < 0:
        raise ValueError("resamp2_route: bad arguments")
    return RESAMP2_ROUTES[r], int(tile.value)


def msresamp_route(t, rate, As, nx):
    """(kernel/class, tile, hm) of the resampler launch of an msresamp's first
    block call of nx inputs; hm: the fused half-band stage's m, 0 if none."""
    tile, hm = C.c_uint(0), C.c_uint(0)
    r = lib().liquid_mi355x_msresamp_route(_KINDS[t], rate, As, nx, C.byref(tile), C.byref(hm))
    if r < 0:
        raise ValueError("msresamp_route: bad arguments")
    return RESAMP_ROUTES[r], int(tile.value), int(hm.value)


def header_functions():
    """Every function the public header declares (macros expanded by cpp)."""
    out = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), HEADER],
                                  text=True)
    names = set()
    for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", out):
        name = m.group(1)
        if name in ("if", "while", "for", "sizeof", "return") or name.startswith("__"):
            continue
        names.add(name)
    # drop typedef'd struct tags and type names that precede '('
    return sorted(n for n in names if not n.endswith("_s") and n not in ("_Complex",))


vp, u, f, i, ull = C.c_void_p, C.c_uint, C.c_float, C.c_int, C.c_ulonglong
FIRDES_DESIGNS = ("rcos", "rrcos", "rkaiser", "arkaiser", "hM3", "gmsktx", "gmskrx", "fexp", "rfexp", "fsech",
                  "rfsech", "farcsech", "rfarcsech")


def _declare(L):
    sig = {}
    for t in (RRRF, CRCF, CCCF):
        tc = cfloat if t == CCCF else f
        sig.update({
            "dotprod_%s_run" % t: (None, [vp, vp, u, vp]),
            "dotprod_%s_run4" % t: (None, [vp, vp, u, vp]),
            "dotprod_%s_create" % t: (vp, [vp, u]),
            "dotprod_%s_recreate" % t: (vp, [vp, vp, u]),
            "dotprod_%s_destroy" % t: (None, [vp]),
            "dotprod_%s_print" % t: (None, [vp]),
            "dotprod_%s_execute" % t: (None, [vp, vp, vp]),
            "dotprod_%s_execute_batch" % t: (None, [vp, vp, ull, vp]),
            "dotprod_%s_execute_batch_dev" % t: (None, [vp, vp, ull, vp]),
            "dotprod_%s_set_stream" % t: (None, [vp, vp]),
            "dotprod_%s_get_stream" % t: (vp, [vp]),
            "firfilt_%s_create" % t: (vp, [vp, u]),
            "firfilt_%s_create_kaiser" % t: (vp, [u, f, f, f]),
            "firfilt_%s_create_rect" % t: (vp, [u]),
            "firfilt_%s_recreate" % t: (vp, [vp, vp, u]),
            "firfilt_%s_destroy" % t: (None, [vp]),
            "firfilt_%s_reset" % t: (None, [vp]),
            "firfilt_%s_print" % t: (None, [vp]),
            "firfilt_%s_set_scale" % t: (None, [vp, tc]),
            "firfilt_%s_push" % t: (None, [vp, f if t == RRRF else cfloat]),
            "firfilt_%s_execute" % t: (None, [vp, vp]),
            "firfilt_%s_execute_block" % t: (None, [vp, vp, u, vp]),
            "firfilt_%s_get_length" % t: (u, [vp]),
            "firfilt_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "firfilt_%s_set_stream" % t: (None, [vp, vp]),
            "firfilt_%s_get_stream" % t: (vp, [vp]),
            "firfilt_%s_synchronize" % t: (None, [vp]),
        })
    for t in (RRRF, CRCF, CCCF):
        ti = f if t == RRRF else cfloat          # sample passed by value
        tc = cfloat if t == CCCF else f          # coefficient / scale by value
        sig.update({
            "firfilt_%s_freqresponse" % t: (None, [vp, f, vp]),
            "firfilt_%s_groupdelay" % t: (f, [vp, f]),
            "firdecim_%s_create" % t: (vp, [u, vp, u]),
            "firdecim_%s_create_kaiser" % t: (vp, [u, u, f]),
            "firdecim_%s_destroy" % t: (None, [vp]),
            "firdecim_%s_print" % t: (None, [vp]),
            "firdecim_%s_clear" % t: (None, [vp]),
            "firdecim_%s_execute" % t: (None, [vp, vp, vp]),
            "firdecim_%s_execute_block" % t: (None, [vp, vp, u, vp]),
            "firdecim_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "firdecim_%s_set_stream" % t: (None, [vp, vp]),
            "firinterp_%s_create" % t: (vp, [u, vp, u]),
            "firinterp_%s_create_kaiser" % t: (vp, [u, u, f]),
            "firinterp_%s_destroy" % t: (None, [vp]),
            "firinterp_%s_print" % t: (None, [vp]),
            "firinterp_%s_reset" % t: (None, [vp]),
            "firinterp_%s_execute" % t: (None, [vp, ti, vp]),
            "firinterp_%s_execute_block" % t: (None, [vp, vp, u, vp]),
            "firinterp_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "firinterp_%s_set_stream" % t: (None, [vp, vp]),
            "resamp_%s_create" % t: (vp, [f, u, f, f, u]),
            "resamp_%s_create_default" % t: (vp, [f]),
            "resamp_%s_destroy" % t: (None, [vp]),
            "resamp_%s_print" % t: (None, [vp]),
            "resamp_%s_reset" % t: (None, [vp]),
            "resamp_%s_get_delay" % t: (u, [vp]),
            "resamp_%s_set_rate" % t: (None, [vp, f]),
            "resamp_%s_adjust_rate" % t: (None, [vp, f]),
            "resamp_%s_execute" % t: (None, [vp, ti, vp, vp]),
            "resamp_%s_execute_block" % t: (None, [vp, vp, u, vp, vp]),
            "resamp_%s_num_output" % t: (ull, [vp, ull]),
            "resamp_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp, vp]),
            "resamp_%s_set_stream" % t: (None, [vp, vp]),
            "resamp_%s_synchronize" % t: (None, [vp]),
            "fftfilt_%s_create" % t: (vp, [vp, u, u]),
            "fftfilt_%s_destroy" % t: (None, [vp]),
            "fftfilt_%s_reset" % t: (None, [vp]),
            "fftfilt_%s_print" % t: (None, [vp]),
            "fftfilt_%s_set_scale" % t: (None, [vp, tc]),
            "fftfilt_%s_execute" % t: (None, [vp, vp, vp]),
            "fftfilt_%s_get_length" % t: (u, [vp]),
            "fftfilt_%s_execute_block" % t: (None, [vp, vp, ull, vp]),
            "fftfilt_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "fftfilt_%s_set_stream" % t: (None, [vp, vp]),
            "firpfb_%s_create" % t: (vp, [u, vp, u]),
            "firpfb_%s_create_kaiser" % t: (vp, [u, u, f, f]),
            "firpfb_%s_recreate" % t: (vp, [vp, u, vp, u]),
            "firpfb_%s_destroy" % t: (None, [vp]),
            "firpfb_%s_print" % t: (None, [vp]),
            "firpfb_%s_set_scale" % t: (None, [vp, tc]),
            "firpfb_%s_reset" % t: (None, [vp]),
            "firpfb_%s_push" % t: (None, [vp, ti]),
            "firpfb_%s_execute" % t: (None, [vp, u, vp]),
            "firpfb_%s_execute_block" % t: (None, [vp, vp, ull, vp]),
            "firpfb_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "firpfb_%s_set_stream" % t: (None, [vp, vp]),
            "firpfb_%s_create_rnyquist" % t: (vp, [i, u, u, u, f]),
            "firpfb_%s_create_drnyquist" % t: (vp, [i, u, u, u, f]),
            "firfilt_%s_create_rnyquist" % t: (vp, [i, u, u, f, f]),
            "firdecim_%s_create_prototype" % t: (vp, [i, u, u, f, f]),
            "firinterp_%s_create_prototype" % t: (vp, [i, u, u, f, f]),
        })
    for t in (RRRF, CRCF, CCCF):
        ti = f if t == RRRF else cfloat
        sig.update({
            "resamp2_%s_create" % t: (vp, [u, f, f]),
            "resamp2_%s_recreate" % t: (vp, [vp, u, f, f]),
            "resamp2_%s_destroy" % t: (None, [vp]),
            "resamp2_%s_print" % t: (None, [vp]),
            "resamp2_%s_clear" % t: (None, [vp]),
            "resamp2_%s_get_delay" % t: (u, [vp]),
            "resamp2_%s_filter_execute" % t: (None, [vp, ti, vp, vp]),
            "resamp2_%s_analyzer_execute" % t: (None, [vp, vp, vp]),
            "resamp2_%s_synthesizer_execute" % t: (None, [vp, vp, vp]),
            "resamp2_%s_decim_execute" % t: (None, [vp, vp, vp]),
            "resamp2_%s_interp_execute" % t: (None, [vp, ti, vp]),
            "resamp2_%s_execute_block" % t: (None, [vp, i, vp, ull, vp, vp]),
            "resamp2_%s_execute_block_dev" % t: (None, [vp, i, vp, ull, vp, vp]),
            "resamp2_%s_set_stream" % t: (None, [vp, vp]),
            "resamp2_%s_synchronize" % t: (None, [vp]),
            "msresamp2_%s_create" % t: (vp, [i, u, f, f, f]),
            "msresamp2_%s_destroy" % t: (None, [vp]),
            "msresamp2_%s_print" % t: (None, [vp]),
            "msresamp2_%s_reset" % t: (None, [vp]),
            "msresamp2_%s_get_delay" % t: (f, [vp]),
            "msresamp2_%s_execute" % t: (None, [vp, vp, vp]),
            "msresamp2_%s_execute_block" % t: (None, [vp, vp, ull, vp]),
            "msresamp2_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "msresamp2_%s_set_stream" % t: (None, [vp, vp]),
            "msresamp2_%s_synchronize" % t: (None, [vp]),
            "msresamp_%s_create" % t: (vp, [f, f]),
            "msresamp_%s_destroy" % t: (None, [vp]),
            "msresamp_%s_print" % t: (None, [vp]),
            "msresamp_%s_reset" % t: (None, [vp]),
            "msresamp_%s_get_delay" % t: (f, [vp]),
            "msresamp_%s_execute" % t: (None, [vp, vp, u, vp, vp]),
            "msresamp_%s_num_output" % t: (ull, [vp, ull]),
            "msresamp_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp, vp]),
            "msresamp_%s_set_stream" % t: (None, [vp, vp]),
            "msresamp_%s_synchronize" % t: (None, [vp]),
        })
    for t, ti in (("spgramcf", cfloat), ("spgramf", f)):
        sig.update({
            t + "_create": (vp, [u, vp, u]),
            t + "_create_kaiser": (vp, [u, u, f]),
            t + "_create_default": (vp, [u]),
            t + "_destroy": (None, [vp]),
            t + "_reset": (None, [vp]),
            t + "_push": (None, [vp, ti]),
            t + "_write": (None, [vp, vp, u]),
            t + "_execute": (None, [vp, vp]),
            t + "_execute_psd": (None, [vp, vp]),
            t + "_accumulate_psd": (None, [vp, vp, f, u]),
            t + "_write_accumulation": (None, [vp, vp]),
            t + "_estimate_psd": (None, [vp, vp, u, vp]),
            t + "_accumulate_psd_dev": (None, [vp, vp, f, ull]),
            t + "_estimate_psd_dev": (None, [vp, vp, ull, vp]),
            t + "_set_stream": (None, [vp, vp]),
            t + "_synchronize": (None, [vp]),
        })
    for t in (CRCF, CCCF):
        sig.update({
            "firpfbch_%s_create" % t: (vp, [i, u, u, vp]),
            "firpfbch_%s_create_kaiser" % t: (vp, [i, u, u, f]),
            "firpfbch_%s_create_rnyquist" % t: (vp, [i, u, u, f, i]),
            "firpfbch_%s_destroy" % t: (None, [vp]),
            "firpfbch_%s_reset" % t: (None, [vp]),
            "firpfbch_%s_print" % t: (None, [vp]),
            "firpfbch_%s_analyzer_execute" % t: (None, [vp, vp, vp]),
            "firpfbch_%s_synthesizer_execute" % t: (None, [vp, vp, vp]),
            "firpfbch_%s_execute_block" % t: (None, [vp, vp, ull, vp]),
            "firpfbch_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "firpfbch_%s_set_stream" % t: (None, [vp, vp]),
        })
    sig.update({
        "firhilbf_create": (vp, [u, f]),
        "firhilbf_destroy": (None, [vp]),
        "firhilbf_print": (None, [vp]),
        "firhilbf_reset": (None, [vp]),
        "firhilbf_r2c_execute": (None, [vp, f, vp]),
        "firhilbf_c2r_execute": (None, [vp, cfloat, vp]),
        "firhilbf_decim_execute": (None, [vp, vp, vp]),
        "firhilbf_decim_execute_block": (None, [vp, vp, u, vp]),
        "firhilbf_interp_execute": (None, [vp, cfloat, vp]),
        "firhilbf_interp_execute_block": (None, [vp, vp, u, vp]),
        "firhilbf_r2c_execute_block": (None, [vp, vp, ull, vp]),
        "firhilbf_c2r_execute_block": (None, [vp, vp, ull, vp]),
        "firhilbf_decim_execute_block_dev": (None, [vp, vp, ull, vp]),
        "firhilbf_interp_execute_block_dev": (None, [vp, vp, ull, vp]),
        "firhilbf_r2c_execute_block_dev": (None, [vp, vp, ull, vp]),
        "firhilbf_c2r_execute_block_dev": (None, [vp, vp, ull, vp]),
        "firhilbf_set_stream": (None, [vp, vp]),
        "firhilbf_synchronize": (None, [vp]),
    })
    for t in (RRRF, CRCF, CCCF):
        ti = f if t == RRRF else cfloat
        sig.update({
            "iirfilt_%s_create" % t: (vp, [vp, u, vp, u]),
            "iirfilt_%s_create_sos" % t: (vp, [vp, vp, u]),
            "iirfilt_%s_create_integrator" % t: (vp, []),
            "iirfilt_%s_create_differentiator" % t: (vp, []),
            "iirfilt_%s_create_dc_blocker" % t: (vp, [f]),
            "iirfilt_%s_create_pll" % t: (vp, [f, f, f]),
            "iirfilt_%s_destroy" % t: (None, [vp]),
            "iirfilt_%s_print" % t: (None, [vp]),
            "iirfilt_%s_reset" % t: (None, [vp]),
            "iirfilt_%s_execute" % t: (None, [vp, ti, vp]),
            "iirfilt_%s_execute_block" % t: (None, [vp, vp, u, vp]),
            "iirfilt_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp]),
            "iirfilt_%s_get_length" % t: (u, [vp]),
            "iirfilt_%s_freqresponse" % t: (None, [vp, f, vp]),
            "iirfilt_%s_groupdelay" % t: (f, [vp, f]),
            "iirfilt_%s_device_eligible" % t: (i, [vp]),
            "iirfilt_%s_set_stream" % t: (None, [vp, vp]),
            "iirfilt_%s_synchronize" % t: (None, [vp]),
        })
        for obj, xarg in (("iirdecim", vp), ("iirinterp", ti)):
            sig.update({
                "%s_%s_create" % (obj, t): (vp, [u, vp, u, vp, u]),
                "%s_%s_create_default" % (obj, t): (vp, [u, u]),
                "%s_%s_create_prototype" % (obj, t): (vp, [u, i, i, i, u, f, f, f, f]),
                "%s_%s_destroy" % (obj, t): (None, [vp]),
                "%s_%s_print" % (obj, t): (None, [vp]),
                "%s_%s_reset" % (obj, t): (None, [vp]),
                "%s_%s_execute" % (obj, t): (None, [vp, xarg, vp]),
                "%s_%s_execute_block" % (obj, t): (None, [vp, vp, u, vp]),
                "%s_%s_execute_block_dev" % (obj, t): (None, [vp, vp, ull, vp]),
                "%s_%s_groupdelay" % (obj, t): (f, [vp, f]),
                "%s_%s_device_eligible" % (obj, t): (i, [vp]),
                "%s_%s_set_stream" % (obj, t): (None, [vp, vp]),
                "%s_%s_synchronize" % (obj, t): (None, [vp]),
            })
    sig.update({
        "iir_group_delay": (f, [vp, u, vp, u, f]),
        "liquid_iirdes": (None, [i, i, i, u, f, f, f, f, vp, vp]),
        "butter_azpkf": (None, [u, vp, vp, vp]),
        "cheby1_azpkf": (None, [u, f, vp, vp, vp]),
        "cheby2_azpkf": (None, [u, f, vp, vp, vp]),
        "ellip_azpkf": (None, [u, f, f, vp, vp, vp]),
        "bessel_azpkf": (None, [u, vp, vp, vp]),
        "iirdes_freqprewarp": (f, [i, f, f]),
        "bilinear_zpkf": (None, [vp, u, vp, u, cfloat, f, vp, vp, vp]),
        "iirdes_dzpk_lp2hp": (None, [vp, vp, u, vp, vp]),
        "iirdes_dzpk_lp2bp": (None, [vp, vp, u, f, vp, vp]),
        "iirdes_dzpk2tff": (None, [vp, vp, u, cfloat, vp, vp]),
        "iirdes_isstable": (i, [vp, vp, u]),
        "liquid_cplxpair": (None, [vp, u, f, vp]),
        "liquid_cplxpair_cleanup": (None, [vp, u, u]),
        "iirdes_dzpk2sosf": (None, [vp, vp, u, cfloat, vp, vp]),
        "iirdes_pll_active_lag": (None, [f, f, f, vp, vp]),
        "iirdes_pll_active_PI": (None, [f, f, f, vp, vp]),
        "liquid_mi355x_iirfilt_run": (u, []),
        "liquid_mi355x_iirfilt_tile": (u, []),
        "liquid_mi355x_iirfilt_scan": (u, []),
        "liquid_mi355x_iirfilt_route": (i, [ull]),
    })
    for t in (CCCF, RRRF):
        sig.update({
            "autocorr_%s_create" % t: (vp, [u, u]),
            "autocorr_%s_destroy" % t: (None, [vp]),
            "autocorr_%s_reset" % t: (None, [vp]),
            "autocorr_%s_print" % t: (None, [vp]),
            "autocorr_%s_push" % t: (None, [vp, f if t == RRRF else cfloat]),
            "autocorr_%s_execute" % t: (None, [vp, vp]),
            "autocorr_%s_execute_block" % t: (None, [vp, vp, u, vp]),
            "autocorr_%s_get_energy" % t: (f, [vp]),
            "autocorr_%s_execute_block_dev" % t: (None, [vp, vp, ull, vp, vp]),
            "autocorr_%s_device_eligible" % t: (i, [vp]),
            "autocorr_%s_set_stream" % t: (None, [vp, vp]),
            "autocorr_%s_synchronize" % t: (None, [vp]),
        })
    sig.update({
        "liquid_mi355x_autocorr_tile": (u, []),
        "liquid_mi355x_autocorr_max_window": (u, []),
        "detector_cccf_create": (vp, [vp, u, f, f]),
        "detector_cccf_destroy": (None, [vp]),
        "detector_cccf_print": (None, [vp]),
        "detector_cccf_reset": (None, [vp]),
        "detector_cccf_correlate": (i, [vp, cfloat, vp, vp, vp]),
        "detector_cccf_correlate_block": (u, [vp, vp, u, vp, vp, vp, vp, u]),
        "detector_cccf_correlate_block_dev": (u, [vp, vp, ull, vp, vp, vp, vp, vp, u]),
        "detector_cccf_get_num_correlators": (u, [vp]),
        "detector_cccf_get_templates": (None, [vp, vp]),
        "detector_cccf_device_eligible": (i, [vp]),
        "detector_cccf_set_stream": (None, [vp, vp]),
        "detector_cccf_synchronize": (None, [vp]),
        "liquid_mi355x_detector_tile": (u, []),
        "liquid_mi355x_detector_max_len": (u, []),
        "liquid_mi355x_detector_max_correlators": (u, []),
        "liquid_mi355x_detector_set_list_capacity": (None, [u]),
        "qdetector_cccf_create": (vp, [vp, u]),
        "qdetector_cccf_create_linear": (vp, [vp, u, i, u, u, f]),
        "qdetector_cccf_destroy": (None, [vp]),
        "qdetector_cccf_print": (None, [vp]),
        "qdetector_cccf_reset": (None, [vp]),
        "qdetector_cccf_execute": (vp, [vp, cfloat]),
        "qdetector_cccf_set_threshold": (None, [vp, f]),
        "qdetector_cccf_set_range": (None, [vp, f]),
        "qdetector_cccf_get_seq_len": (u, [vp]),
        "qdetector_cccf_get_sequence": (vp, [vp]),
        "qdetector_cccf_get_buf_len": (u, [vp]),
        "qdetector_cccf_get_tau": (f, [vp]),
        "qdetector_cccf_get_gamma": (f, [vp]),
        "qdetector_cccf_get_dphi": (f, [vp]),
        "qdetector_cccf_get_phi": (f, [vp]),
        "qdetector_cccf_execute_block": (u, [vp, vp, ull, u, vp, vp, vp, vp, vp, vp, vp, vp]),
        "qdetector_cccf_execute_block_dev": (u, [vp, vp, ull, u, vp, vp, vp, vp, vp, vp, vp, vp]),
        "qdetector_cccf_get_range": (i, [vp]),
        "qdetector_cccf_get_threshold": (f, [vp]),
        "qdetector_cccf_set_stream": (None, [vp, vp]),
        "qdetector_cccf_synchronize": (None, [vp]),
        "liquid_mi355x_qdetector_route": (i, [u, i, ull]),
        "liquid_mi355x_qdetector_set_chunk": (None, [u]),
        "liquid_mi355x_qdetector_set_route": (None, [i]),
        "liquid_mi355x_qdetector_chunk": (u, [u]),
    })
    sig.update({
        "nco_crcf_create": (vp, [i]),
        "nco_crcf_destroy": (None, [vp]),
        "nco_crcf_print": (None, [vp]),
        "nco_crcf_reset": (None, [vp]),
        "nco_crcf_get_frequency": (f, [vp]),
        "nco_crcf_set_frequency": (None, [vp, f]),
        "nco_crcf_adjust_frequency": (None, [vp, f]),
        "nco_crcf_get_phase": (f, [vp]),
        "nco_crcf_set_phase": (None, [vp, f]),
        "nco_crcf_adjust_phase": (None, [vp, f]),
        "nco_crcf_step": (None, [vp]),
        "nco_crcf_sin": (f, [vp]),
        "nco_crcf_cos": (f, [vp]),
        "nco_crcf_sincos": (None, [vp, vp, vp]),
        "nco_crcf_cexpf": (None, [vp, vp]),
        "nco_crcf_pll_set_bandwidth": (None, [vp, f]),
        "nco_crcf_pll_step": (None, [vp, f]),
        "nco_crcf_mix_up": (None, [vp, cfloat, vp]),
        "nco_crcf_mix_down": (None, [vp, cfloat, vp]),
        "nco_crcf_mix_block_up": (None, [vp, vp, vp, u]),
        "nco_crcf_mix_block_down": (None, [vp, vp, vp, u]),
        "nco_crcf_mix_block_up_dev": (None, [vp, vp, vp, ull]),
        "nco_crcf_mix_block_down_dev": (None, [vp, vp, vp, ull]),
        "nco_crcf_device_eligible": (i, [vp]),
        "nco_crcf_set_stream": (None, [vp, vp]),
        "nco_crcf_synchronize": (None, [vp]),
        "liquid_unwrap_phase": (None, [vp, u]),
        "liquid_unwrap_phase2": (None, [vp, u]),
        "liquid_mi355x_nco_tile": (u, []),
        "liquid_mi355x_nco_checkpoint": (u, []),
        "liquid_mi355x_nco_walk": (C.c_longlong, [i, f, f, ull, i, vp, vp, vp, vp]),
        "freqmod_create": (vp, [f]),
        "freqmod_destroy": (None, [vp]),
        "freqmod_print": (None, [vp]),
        "freqmod_reset": (None, [vp]),
        "freqmod_modulate": (None, [vp, f, vp]),
        "freqmod_modulate_block": (None, [vp, vp, u, vp]),
        "freqmod_modulate_block_dev": (None, [vp, vp, ull, vp]),
        "freqmod_get_phase": (u, [vp]),
        "freqmod_get_table": (None, [vp, vp]),
        "freqmod_set_stream": (None, [vp, vp]),
        "freqmod_synchronize": (None, [vp]),
        "freqdem_create": (vp, [f]),
        "freqdem_create_channels": (vp, [f, u]),
        "freqdem_get_channels": (u, [vp]),
        "freqdem_destroy": (None, [vp]),
        "freqdem_print": (None, [vp]),
        "freqdem_reset": (None, [vp]),
        "freqdem_demodulate": (None, [vp, cfloat, vp]),
        "freqdem_demodulate_block": (None, [vp, vp, u, vp]),
        "freqdem_demodulate_block_dev": (None, [vp, vp, ull, vp]),
        "freqdem_set_stream": (None, [vp, vp]),
        "freqdem_synchronize": (None, [vp]),
        "liquid_mi355x_freqmod_tile": (u, []),
        "liquid_mi355x_freqmod_scan_pass": (u, []),
        "liquid_mi355x_freqdem_tile": (u, []),
        "liquid_mi355x_freqdem_switch": (u, []),
        "liquid_mi355x_freqdem_frames": (u, []),
    })
    for d in FIRDES_DESIGNS:
        sig["liquid_firdes_" + d] = (None, [u, u, f, f, vp])
    sig.update({
        "liquid_firdes_kaiser": (None, [u, f, f, f, vp]),
        "kaiser_beta_As": (f, [f]),
        "liquid_libversion_number": (i, []),
        "liquid_mi355x_malloc": (vp, [ull]),
        "liquid_mi355x_free": (None, [vp]),
        "liquid_mi355x_memcpy_h2d": (None, [vp, vp, ull]),
        "liquid_mi355x_memcpy_d2h": (None, [vp, vp, ull]),
        "liquid_mi355x_device_synchronize": (None, []),
        "liquid_mi355x_set_max_workgroups": (None, [u]),
        "liquid_mi355x_get_max_workgroups": (u, []),
        "liquid_mi355x_firpfbch2_route": (i, [i, u, u, ull, i, i, i, i, vp, vp, vp]),
        "liquid_mi355x_firpfbch_route": (i, [i, i, u, u, ull, i, i, i, vp, vp, vp]),
        "liquid_mi355x_channelizer_route_count": (i, []),
        "liquid_mi355x_channelizer_route_name": (C.c_char_p, [i]),
        "liquid_mi355x_set_channelizer_chunk": (i, [ull]),
        "liquid_mi355x_get_channelizer_chunk": (ull, []),
        "liquid_mi355x_pinned_input_max": (u, []),
        "liquid_mi355x_copyout_max": (u, []),
        "liquid_mi355x_dotprod_route": (i, [i, u, i, ull]),
        "liquid_mi355x_dotprod_blocks": (u, [i, u, i, ull]),
        "liquid_mi355x_dotprod_block_cap": (u, []),
        "liquid_mi355x_firdecim_route": (i, [i, u, u, i, ull]),
        "liquid_mi355x_firdecim_tile": (u, [i]),
        "liquid_mi355x_firdecim_grid_cap": (u, [i, u, u, i]),
        "liquid_mi355x_firinterp_route": (i, [i, u, u, i]),
        "liquid_mi355x_firinterp_max_taps": (u, [i]),
        "liquid_mi355x_fft_route": (i, [u, i]),
        "liquid_mi355x_spgram_route": (i, [i, u, u, ull]),
        "liquid_mi355x_spgram_chunk": (u, []),
        "liquid_mi355x_spgram_fold_group": (u, []),
        "liquid_mi355x_spgram_batch_samples": (ull, []),
        "liquid_mi355x_resamp_route": (i, [i, f, u, u, ull, vp]),
        "liquid_mi355x_resamp2_route": (i, [i, u, ull, vp]),
        "liquid_mi355x_msresamp_route": (i, [i, f, f, ull, vp, vp]),
        "kaiser": (f, [u, u, f, f]),
        "hann": (f, [u, u]),
        "blackmanharris": (f, [u, u]),
        "liquid_rcostaper_windowf": (f, [u, u, u]),
        "liquid_kbd": (f, [u, u, f]),
        "liquid_kbd_window": (None, [u, f, vp]),
        "fft_create_plan": (vp, [u, vp, vp, i, i]),
        "fft_create_plan_r2r_1d": (vp, [u, vp, vp, i, i]),
        "fft_destroy_plan": (None, [vp]),
        "fft_print_plan": (None, [vp]),
        "fft_execute": (None, [vp]),
        "fft_run": (None, [u, vp, vp, i, i]),
        "fft_r2r_1d_run": (None, [u, vp, vp, i, i]),
        "fft_shift": (None, [vp, u]),
        "liquid_nextpow2": (u, [u]),
        "fft_execute_batch": (None, [vp, vp, vp, ull]),
        "fft_execute_batch_dev": (None, [vp, vp, vp, ull]),
        "fft_set_stream": (None, [vp, vp]),
        "liquid_firdes_prototype": (None, [i, u, u, f, f, vp]),
        "liquid_getopt_str2firfilt": (i, [C.c_char_p]),
        "estimate_req_filter_len": (u, [f, f]),
        "estimate_req_filter_As": (f, [f, u]),
        "estimate_req_filter_df": (f, [f, u]),
        "rkaiser_approximate_rho": (f, [u, f]),
        "firdespm_run": (None, [u, u, vp, vp, vp, vp, i, vp]),
        "liquid_filter_autocorr": (f, [vp, u, i]),
        "liquid_filter_isi": (None, [vp, u, u, vp, vp]),
        "liquid_Qf": (f, [f]),
        "firpfbch2_crcf_create": (vp, [i, u, u, vp]),
        "firpfbch2_crcf_create_kaiser": (vp, [i, u, u, f]),
        "firpfbch2_crcf_destroy": (None, [vp]),
        "firpfbch2_crcf_reset": (None, [vp]),
        "firpfbch2_crcf_execute": (None, [vp, vp, vp]),
        "firpfbch2_crcf_execute_block": (None, [vp, vp, ull, vp]),
        "firpfbch2_crcf_execute_block_dev": (None, [vp, vp, ull, vp]),
        "firpfbch2_crcf_set_stream": (None, [vp, vp]),
        "firpfbch2_crcf_get_stream": (vp, [vp]),
        "firpfbch2_crcf_synchronize": (None, [vp]),
    })
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ filter design (liquid.h:1413-1668)
FIRFILT_TYPES = ["kaiser", "pm", "rcos", "fexp", "fsech", "farcsech", "arkaiser", "rkaiser", "rrc", "hM3",
                 "gmsktx", "gmskrx", "rfexp", "rfsech", "rfarcsech"]
LIQUID_FIRFILT = {n: k + 1 for k, n in enumerate(FIRFILT_TYPES)}


def firdes_prototype(ftype, k, m, beta, dt=0.0):
    """liquid_firdes_prototype: 2km+1 taps (ftype: name or LIQUID_FIRFILT_* code)."""
    code = LIQUID_FIRFILT[ftype] if isinstance(ftype, str) else int(ftype)
    h = np.zeros(2 * k * m + 1, np.float32)
    lib().liquid_firdes_prototype(code, k, m, beta, dt, ptr(h))
    return h


def firdes(design, k, m, beta, dt=0.0):
    """liquid_firdes_<design>(k, m, beta, dt): e.g. design = "rkaiser", "rcos", "gmskrx"."""
    h = np.zeros(2 * k * m + 1, np.float32)
    getattr(lib(), "liquid_firdes_" + design)(k, m, beta, dt, ptr(h))
    return h


def firdespm(n, bands, des, weights=None, wtype=None):
    """firdespm_run, band-pass designs."""
    bands = np.ascontiguousarray(bands, np.float32)
    des = np.ascontiguousarray(des, np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    wt = None if wtype is None else np.ascontiguousarray(wtype, np.int32)
    h = np.zeros(n, np.float32)
    lib().firdespm_run(n, len(des), ptr(bands), ptr(des), None if w is None else ptr(w),
                       None if wt is None else ptr(wt), 0, ptr(h))
    return h


def filter_isi(h, k, m):
    h = np.ascontiguousarray(h, np.float32)
    rms, mx = C.c_float(), C.c_float()
    lib().liquid_filter_isi(ptr(h), k, m, C.byref(rms), C.byref(mx))
    return rms.value, mx.value


def _samples(x, t):
    return np.ascontiguousarray(x, dtype=np.float32 if t == RRRF else np.complex64)


def _coefs(h, t):
    return np.ascontiguousarray(h, dtype=np.complex64 if t == CCCF else np.float32)


# ------------------------------------------------------------------ device buffers
class DeviceBuffer:
    """Device allocation made through the library (liquid_mi355x_malloc)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.p = lib().liquid_mi355x_malloc(self.nbytes)

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        lib().liquid_mi355x_memcpy_h2d(b.p, ptr(a), a.nbytes)
        return b

    def to_array(self, dtype, count):
        a = np.empty(count, dtype)
        lib().liquid_mi355x_memcpy_d2h(ptr(a), self.p, a.nbytes)
        return a

    def free(self):
        if self.p:
            lib().liquid_mi355x_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def firdes_kaiser(n, fc, As, mu=0.0):
    h = np.zeros(n, np.float32)
    lib().liquid_firdes_kaiser(n, fc, As, mu, ptr(h))
    return h


# ------------------------------------------------------------------ objects
class _Obj:
    prefix = None

    def _fn(self, name):
        return getattr(lib(), self.prefix + name)

    def destroy(self):
        if getattr(self, "q", None):
            self._fn("_destroy")(self.q)
            self.q = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def set_stream(self, s):
        self._fn("_set_stream")(self.q, s)

    @classmethod
    def construct(cls, ctor, args, t=CRCF, **attrs):
        """Object from another constructor of the family, e.g.
        FirFilt.construct("_create_rnyquist", (type, k, m, beta, mu), t=CRCF)."""
        o = cls.__new__(cls)
        o.t = t
        o.prefix = cls.family % t
        o.__dict__.update(attrs)
        o.q = getattr(lib(), o.prefix + ctor)(*args)
        if not o.q:
            raise RuntimeError(o.prefix + ctor + " failed")
        return o


class FirFilt(_Obj):
    family = "firfilt_%s"

    def freqresponse(self, fc):
        H = cfloat(0.0, 0.0)
        self._fn("_freqresponse")(self.q, fc, C.byref(H))
        return complex(H.re, H.im) if hasattr(H, "re") else complex(H.real, H.imag)

    def groupdelay(self, fc):
        return float(self._fn("_groupdelay")(self.q, fc))

    def __init__(self, t, h=None, kaiser=None):
        self.t = t
        self.prefix = "firfilt_%s" % t
        if kaiser is not None:
            self.q = self._fn("_create_kaiser")(*kaiser)
        else:
            self._h = _coefs(h, t)
            self.q = self._fn("_create")(ptr(self._h), len(self._h))

    def set_scale(self, s):
        if self.t == CCCF:
            s = complex(s)
            self._fn("_set_scale")(self.q, cfloat(s.real, s.imag))
        else:
            self._fn("_set_scale")(self.q, float(s))

    def reset(self):
        self._fn("_reset")(self.q)

    def push(self, v):
        if self.t == RRRF:
            self._fn("_push")(self.q, float(v))
        else:
            v = complex(v)
            self._fn("_push")(self.q, cfloat(v.real, v.imag))

    def execute(self):
        y = _samples([0], self.t)
        self._fn("_execute")(self.q, ptr(y))
        return y[0]

    def execute_block(self, x):
        x = _samples(x, self.t)
        y = np.zeros_like(x)
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def execute_block_dev(self, dx, n, dy):
        self._fn("_execute_block_dev")(self.q, dx, n, dy)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_length(self):
        return self._fn("_get_length")(self.q)


class DotProd(_Obj):
    def __init__(self, t, h):
        self.t = t
        self.prefix = "dotprod_%s" % t
        self._h = _coefs(h, t)
        self.n = len(self._h)
        self.q = self._fn("_create")(ptr(self._h), self.n)

    def execute(self, x):
        x = _samples(x, self.t)
        y = _samples([0], self.t)
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y[0]

    def recreate(self, h):
        """dotprod_*_recreate: new coefficients, of any length, on the same object."""
        self._h = _coefs(h, self.t)
        self.n = len(self._h)
        self.q = self._fn("_recreate")(self.q, ptr(self._h), self.n)

    def execute_batch(self, X, nvec=None, fill=0):
        """nvec: the number of rows where the length does not tell (n = 0);
        fill: what the result array holds before the call."""
        X = _samples(X, self.t)
        if nvec is None:
            nvec = X.size // self.n
        Y = np.full(nvec, fill, X.dtype)
        self._fn("_execute_batch")(self.q, ptr(X), nvec, ptr(Y))
        return Y

    def execute_batch_dev(self, dX, nvec, dY):
        self._fn("_execute_batch_dev")(self.q, dX, nvec, dY)


def dotprod_run(t, h, x, fn="run"):
    h = _coefs(h, t)
    x = _samples(x, t)
    y = _samples([0], t)
    getattr(lib(), "dotprod_%s_%s" % (t, fn))(ptr(h), ptr(x), len(h), ptr(y))
    return y[0]


def dotprod_run4(t, h, x):
    return dotprod_run(t, h, x, "run4")


def _by_value(v, t):
    if t == RRRF:
        return float(np.real(v))
    v = complex(v)
    return cfloat(v.real, v.imag)


def _out_dtype(t):
    return np.float32 if t == RRRF else np.complex64


class FirDecim(_Obj):
    family = "firdecim_%s"

    def __init__(self, M, h=None, m=None, As=None, t=CRCF):
        self.M, self.t = M, t
        self.prefix = "firdecim_%s" % t
        if h is None:
            self.q = self._fn("_create_kaiser")(M, m, As)
        else:
            self._h = _coefs(h, t)
            self.q = self._fn("_create")(M, ptr(self._h), len(self._h))

    def execute_block(self, x):
        x = _samples(x, self.t)
        n = len(x) // self.M
        y = np.zeros(n, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), n, ptr(y))
        return y

    def execute(self, x):
        x = _samples(x, self.t)
        y = np.zeros(1, _out_dtype(self.t))
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y[0]

    def clear(self):
        self._fn("_clear")(self.q)


class FirInterp(_Obj):
    family = "firinterp_%s"

    def __init__(self, M, h=None, m=None, As=None, t=CRCF):
        self.M, self.t = M, t
        self.prefix = "firinterp_%s" % t
        if h is None:
            self.q = self._fn("_create_kaiser")(M, m, As)
        else:
            self._h = _coefs(h, t)
            self.q = self._fn("_create")(M, ptr(self._h), len(self._h))

    def execute_block(self, x):
        x = _samples(x, self.t)
        y = np.zeros(len(x) * self.M, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def execute(self, v):
        y = np.zeros(self.M, _out_dtype(self.t))
        self._fn("_execute")(self.q, _by_value(v, self.t), ptr(y))
        return y

    def reset(self):
        self._fn("_reset")(self.q)

    def execute_block_dev(self, dx, n, dy):
        self._fn("_execute_block_dev")(self.q, dx, n, dy)

    def synchronize(self):
        lib().liquid_mi355x_device_synchronize()


class FftFilt(_Obj):
    family = "fftfilt_%s"

    def __init__(self, h, n, t=CRCF):
        self.n, self.t = n, t
        self.prefix = "fftfilt_%s" % t
        self._h = _coefs(h, t)
        self.q = self._fn("_create")(ptr(self._h), len(self._h), n)

    def set_scale(self, s):
        self._fn("_set_scale")(self.q, _by_value(s, CCCF) if self.t == CCCF else float(np.real(s)))

    def reset(self):
        self._fn("_reset")(self.q)

    def execute(self, x):
        x = _samples(x, self.t)
        assert len(x) == self.n
        y = np.zeros_like(x)
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y

    def execute_block(self, x):
        x = _samples(x, self.t)
        y = np.zeros_like(x)
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def execute_block_dev(self, dx, n, dy):
        self._fn("_execute_block_dev")(self.q, dx, n, dy)


class FirPfbch(_Obj):
    family = "firpfbch_%s"

    def __init__(self, typ, M, p=None, h=None, m=None, As=None, t=CRCF, rnyquist=None):
        self.typ, self.M, self.t = typ, M, t
        self.prefix = self.family % t
        if rnyquist is not None:               # (m, beta, ftype)
            self.q = self._fn("_create_rnyquist")(typ, M, rnyquist[0], rnyquist[1], rnyquist[2])
        elif h is None:
            self.q = self._fn("_create_kaiser")(typ, M, m, As)
        else:
            self._h = _coefs(h, t)
            self.q = self._fn("_create")(typ, M, p, ptr(self._h))

    def execute(self, x):
        x = _samples(x, CRCF)
        y = np.zeros(self.M, np.complex64)
        fn = "_analyzer_execute" if self.typ == LIQUID_ANALYZER else "_synthesizer_execute"
        self._fn(fn)(self.q, ptr(x), ptr(y))
        return y

    def execute_block(self, x):
        x = _samples(x, CRCF)
        nb = len(x) // self.M
        y = np.zeros(nb * self.M, np.complex64)
        self._fn("_execute_block")(self.q, ptr(x), nb, ptr(y))
        return y

    def reset(self):
        self._fn("_reset")(self.q)

    def execute_block_dev(self, dx, nblocks, dy):
        self._fn("_execute_block_dev")(self.q, dx, nblocks, dy)

    def synchronize(self):
        lib().liquid_mi355x_device_synchronize()


class FirPfbch2(_Obj):
    prefix = "firpfbch2_crcf"

    def __init__(self, typ, M, m, As=None, h=None):
        self.typ, self.M, self.m = typ, M, m
        if h is None:
            self.q = self._fn("_create_kaiser")(typ, M, m, As)
        else:
            self._h = _coefs(h, CRCF)
            self.q = self._fn("_create")(typ, M, m, ptr(self._h))
        self.nin = M // 2 if typ == LIQUID_ANALYZER else M
        self.nout = M if typ == LIQUID_ANALYZER else M // 2

    def reset(self):
        self._fn("_reset")(self.q)

    def execute(self, x):
        x = _samples(x, CRCF)
        y = np.zeros(self.nout, np.complex64)
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y

    def execute_block(self, x):
        x = _samples(x, CRCF)
        nb = len(x) // self.nin
        y = np.zeros(nb * self.nout, np.complex64)
        self._fn("_execute_block")(self.q, ptr(x), nb, ptr(y))
        return y

    def execute_block_dev(self, dx, nblocks, dy):
        self._fn("_execute_block_dev")(self.q, dx, nblocks, dy)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_stream(self):
        return self._fn("_get_stream")(self.q)


class FirPfb(_Obj):
    family = "firpfb_%s"

    def __init__(self, M, h=None, m=None, fc=None, As=None, t=CRCF):
        self.M, self.t = M, t
        self.prefix = "firpfb_%s" % t
        if h is None:
            self.q = self._fn("_create_kaiser")(M, m, fc, As)
        else:
            self._h = _coefs(h, t)
            self.q = self._fn("_create")(M, ptr(self._h), len(self._h))

    def set_scale(self, s):
        self._fn("_set_scale")(self.q, _by_value(s, CCCF) if self.t == CCCF else float(np.real(s)))

    def reset(self):
        self._fn("_reset")(self.q)

    def push(self, v):
        self._fn("_push")(self.q, _by_value(v, self.t))

    def execute(self, i):
        y = np.zeros(1, _out_dtype(self.t))
        self._fn("_execute")(self.q, i, ptr(y))
        return y[0]

    def execute_block(self, x):
        """push each x[t] and evaluate every bank: returns (len(x), M)"""
        x = _samples(x, self.t)
        y = np.zeros(len(x) * self.M, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y.reshape(len(x), self.M)

    def execute_block_dev(self, dx, n, dy):
        """n inputs at dx -> n * M outputs at dy, y[t * M + i] (device pointers)"""
        self._fn("_execute_block_dev")(self.q, dx, n, dy)

    def synchronize(self):
        lib().liquid_mi355x_device_synchronize()


class Resamp(_Obj):
    family = "resamp_%s"

    def __init__(self, rate, m=None, fc=None, As=None, npfb=None, t=CRCF):
        self.t = t
        self.prefix = "resamp_%s" % t
        if m is None:
            self.q = self._fn("_create_default")(rate)
        else:
            self.q = self._fn("_create")(rate, m, fc, As, npfb)

    def reset(self):
        self._fn("_reset")(self.q)

    def set_rate(self, r):
        self._fn("_set_rate")(self.q, float(r))

    def adjust_rate(self, d):
        self._fn("_adjust_rate")(self.q, float(d))

    def get_delay(self):
        return self._fn("_get_delay")(self.q)

    def num_output(self, nx):
        return int(self._fn("_num_output")(self.q, nx))

    def execute(self, v):
        y = np.zeros(max(1, self.num_output(1)), _out_dtype(self.t))
        nw = C.c_uint(0)
        self._fn("_execute")(self.q, _by_value(v, self.t), ptr(y), C.byref(nw))
        return y[:nw.value].copy()

    def execute_block(self, x):
        x = _samples(x, self.t)
        y = np.zeros(max(1, self.num_output(len(x))), _out_dtype(self.t))
        ny = C.c_uint(0)
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y), C.byref(ny))
        return y[:ny.value]

    def execute_block_dev(self, dx, nx, dy):
        ny = C.c_ulonglong(0)
        self._fn("_execute_block_dev")(self.q, dx, nx, dy, C.byref(ny))
        return ny.value

    def synchronize(self):
        self._fn("_synchronize")(self.q)


# ------------------------------------------------------------------ half-band / multi-stage resamplers
RESAMP2_FILTER, RESAMP2_ANALYZER, RESAMP2_SYNTHESIZER, RESAMP2_DECIM, RESAMP2_INTERP = range(5)
LIQUID_RESAMP_INTERP, LIQUID_RESAMP_DECIM = 0, 1


class Resamp2(_Obj):
    family = "resamp2_%s"
    NIN = {0: 1, 1: 2, 2: 2, 3: 2, 4: 1}
    NOUT = {0: 1, 1: 2, 2: 2, 3: 1, 4: 2}

    def __init__(self, m, f0, As, t=CRCF):
        self.t = t
        self.prefix = self.family % t
        self.q = self._fn("_create")(m, f0, As)

    def clear(self):
        self._fn("_clear")(self.q)

    def get_delay(self):
        return self._fn("_get_delay")(self.q)

    def run(self, mode, x):
        """n consecutive calls of one mode (execute_block extension)."""
        x = _samples(x, self.t)
        n = len(x) // self.NIN[mode]
        y0 = np.zeros(n * self.NOUT[mode], _out_dtype(self.t))
        y1 = np.zeros(n, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, mode, ptr(x), n, ptr(y0), ptr(y1))
        return (y0, y1) if mode == RESAMP2_FILTER else y0

    def run_dev(self, mode, dx, n, dy0, dy1=None):
        """n consecutive calls of one mode on device pointers."""
        self._fn("_execute_block_dev")(self.q, mode, dx, n, dy0, dy1)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def call(self, mode, x):
        """one call of the original per-call API"""
        if mode == RESAMP2_FILTER:
            y0, y1 = np.zeros(1, _out_dtype(self.t)), np.zeros(1, _out_dtype(self.t))
            self._fn("_filter_execute")(self.q, _by_value(x, self.t), ptr(y0), ptr(y1))
            return y0[0], y1[0]
        if mode == RESAMP2_INTERP:
            y = np.zeros(2, _out_dtype(self.t))
            self._fn("_interp_execute")(self.q, _by_value(x, self.t), ptr(y))
            return y
        x = _samples(x, self.t)
        y = np.zeros(self.NOUT[mode], _out_dtype(self.t))
        fn = {RESAMP2_ANALYZER: "_analyzer_execute", RESAMP2_SYNTHESIZER: "_synthesizer_execute",
              RESAMP2_DECIM: "_decim_execute"}[mode]
        self._fn(fn)(self.q, ptr(x), ptr(y))
        return y


class FirHilb(_Obj):
    """firhilbf: Hilbert transform filter, 2:1 decimator (real -> complex) and
    interpolator (complex -> real); 4m+1 taps, delay 2m+1."""
    prefix = "firhilbf"
    TILE = 1024   # calls per workgroup of the block kernels (LQK_FIRHILB_TILE)

    def __init__(self, m, As):
        self.m = m
        self.q = self._fn("_create")(m, As)

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def decim_block(self, x):
        """len(x) // 2 decim calls: real x -> complex y"""
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros(len(x) // 2, np.complex64)
        self._fn("_decim_execute_block")(self.q, ptr(x), len(y), ptr(y))
        return y

    def interp_block(self, x):
        """len(x) interp calls: complex x -> 2 len(x) real y"""
        x = np.ascontiguousarray(x, np.complex64)
        y = np.zeros(2 * len(x), np.float32)
        self._fn("_interp_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def r2c_block(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros(len(x), np.complex64)
        self._fn("_r2c_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def c2r_block(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        y = np.zeros(len(x), np.float32)
        self._fn("_c2r_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def decim(self, x):
        """one call of the original API: two real samples -> one complex"""
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros(1, np.complex64)
        self._fn("_decim_execute")(self.q, ptr(x), ptr(y))
        return y[0]

    def interp(self, v):
        y = np.zeros(2, np.float32)
        self._fn("_interp_execute")(self.q, _by_value(v, CRCF), ptr(y))
        return y

    def r2c(self, v):
        y = np.zeros(1, np.complex64)
        self._fn("_r2c_execute")(self.q, float(v), ptr(y))
        return y[0]

    def c2r(self, v):
        y = np.zeros(1, np.float32)
        self._fn("_c2r_execute")(self.q, _by_value(v, CRCF), ptr(y))
        return y[0]

    # device pointers; n counts calls (input and output must not overlap)
    def decim_block_dev(self, dx, n, dy):
        self._fn("_decim_execute_block_dev")(self.q, dx, n, dy)

    def interp_block_dev(self, dx, n, dy):
        self._fn("_interp_execute_block_dev")(self.q, dx, n, dy)

    def r2c_block_dev(self, dx, n, dy):
        self._fn("_r2c_execute_block_dev")(self.q, dx, n, dy)

    def c2r_block_dev(self, dx, n, dy):
        self._fn("_c2r_execute_block_dev")(self.q, dx, n, dy)


class _LibConst:
    """a class attribute read from the library on first use"""

    def __init__(self, fn):
        self.fn = fn

    def __get__(self, obj, owner):
        return int(getattr(lib(), self.fn)())


class IirFilt(_Obj):
    """iirfilt_<t>: recursive filter.  IirFilt(t, b, a) is the numerator /
    denominator form (create); the classmethods are the other constructors.
    Block calls run on the GPU when device_eligible, else in the library's
    host loop."""
    family = "iirfilt_%s"
    RUN = _LibConst("liquid_mi355x_iirfilt_run")     # consecutive samples per lane
    TILE = _LibConst("liquid_mi355x_iirfilt_tile")   # samples per workgroup
    SCAN = _LibConst("liquid_mi355x_iirfilt_scan")   # tiles per block of the cross-tile scan

    def __init__(self, t, b, a):
        self.t = t
        self.prefix = self.family % t
        self._b, self._a = _coefs(b, t), _coefs(a, t)
        self.q = self._fn("_create")(ptr(self._b), len(self._b), ptr(self._a), len(self._a))

    @classmethod
    def sos(cls, t, B, A):
        """create_sos: B, A of 3 coefficients per section"""
        B, A = _coefs(B, t).ravel(), _coefs(A, t).ravel()
        assert len(B) == len(A) and len(B) % 3 == 0
        return cls.construct("_create_sos", (ptr(B), ptr(A), len(B) // 3), t=t, _b=B, _a=A)

    @classmethod
    def prototype(cls, t, ftype, btype, fmt, order, fc, f0=0.0, Ap=0.1, As=60.0):
        """the liquid_iirdes design (names or LIQUID_IIRDES_* codes) handed to create_sos (sos) or
        create (tf): what the reference's create_prototype does, which the library does not export"""
        B, A = iirdes(ftype, btype, fmt, order, fc, f0, Ap, As)
        return cls.sos(t, B, A) if _iirdes_codes(ftype, btype, fmt)[2] == 0 else cls(t, B, A)

    @classmethod
    def lowpass(cls, t, order, fc):
        """Butterworth low-pass, SOS form (the reference's create_lowpass)"""
        return cls.prototype(t, "butter", "lowpass", "sos", order, fc, 0.0, 0.1, 60.0)

    @classmethod
    def dc_blocker(cls, t, alpha):
        return cls.construct("_create_dc_blocker", (alpha,), t=t)

    @classmethod
    def pll(cls, t, w, zeta, K):
        return cls.construct("_create_pll", (w, zeta, K), t=t)

    @classmethod
    def integrator(cls, t):
        return cls.construct("_create_integrator", (), t=t)

    @classmethod
    def differentiator(cls, t):
        return cls.construct("_create_differentiator", (), t=t)

    @property
    def device_eligible(self):
        return bool(self._fn("_device_eligible")(self.q))

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_length(self):
        return int(self._fn("_get_length")(self.q))

    def execute(self, v):
        y = np.zeros(1, _out_dtype(self.t))
        self._fn("_execute")(self.q, _by_value(v, self.t), ptr(y))
        return y[0]

    def execute_block(self, x):
        x = _samples(x, self.t)
        y = np.zeros(len(x), _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y

    def execute_block_dev(self, dx, n, dy):
        self._fn("_execute_block_dev")(self.q, dx, n, dy)

    def freqresponse(self, fc):
        H = np.zeros(1, np.complex64)
        self._fn("_freqresponse")(self.q, fc, ptr(H))
        return complex(H[0])

    def groupdelay(self, fc):
        return float(self._fn("_groupdelay")(self.q, fc))


class AutoCorr(_Obj):
    """autocorr_<kind>: windowed delay autocorrelation, kind "cccf" or "rrrf".
    rxx[n] = sum_{k=n-W+1..n} x[k] conj(x[k-d]); block calls run on the GPU when
    device_eligible (window <= MAX_WINDOW), else in the library's host loop."""
    family = "autocorr_%s"
    TILE = _LibConst("liquid_mi355x_autocorr_tile")               # outputs per workgroup
    MAX_WINDOW = _LibConst("liquid_mi355x_autocorr_max_window")   # the largest window the kernel takes

    def __init__(self, kind, window, delay):
        assert kind in (CCCF, RRRF)
        self.t, self.window, self.delay = kind, int(window), int(delay)
        self.prefix = self.family % kind
        self.q = self._fn("_create")(self.window, self.delay)

    @property
    def device_eligible(self):
        return bool(self._fn("_device_eligible")(self.q))

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def push(self, v):
        self._fn("_push")(self.q, _by_value(v, self.t))

    def execute(self):
        y = np.zeros(1, _out_dtype(self.t))
        self._fn("_execute")(self.q, ptr(y))
        return y[0]

    def execute_block(self, x, inplace=False):
        """rxx of the samples x; inplace: the library writes over its input array"""
        x = _samples(x, self.t)
        y = x.copy() if inplace else np.zeros(len(x), _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(y) if inplace else ptr(x), len(x), ptr(y))
        return y

    def execute_block_dev(self, dx, n, drxx, de2=0):
        """device pointers; de2 = 0: no energy output"""
        self._fn("_execute_block_dev")(self.q, dx, n, drxx, de2 or None)

    def get_energy(self):
        return float(self._fn("_get_energy")(self.q))


def set_detector_list_capacity(records):
    """Records the detector's device list holds (0: the default).  For tests."""
    lib().liquid_mi355x_detector_set_list_capacity(int(records))


class Detector(_Obj):
    """detector_cccf: preamble correlator bank over the sequence s.  correlate()
    runs on the host (the constructor needs no GPU); the block calls run on the
    GPU when device_eligible, else in the library's host loop.  A detection is
    (index, tau_hat, dphi_hat, gamma_hat); the block calls return (count,
    index, tau_hat, dphi_hat, gamma_hat) with arrays of min(count, max_det)."""
    prefix = "detector_cccf"
    TILE = _LibConst("liquid_mi355x_detector_tile")                         # outputs per workgroup
    MAX_LEN = _LibConst("liquid_mi355x_detector_max_len")                   # the longest sequence the kernel takes
    MAX_CORRELATORS = _LibConst("liquid_mi355x_detector_max_correlators")   # the widest bank it takes

    def __init__(self, s, threshold, dphi_max):
        self.s = _samples(s, CCCF)
        self.n = len(self.s)
        self.q = self._fn("_create")(ptr(self.s), self.n, float(threshold), float(dphi_max))

    @property
    def device_eligible(self):
        return bool(self._fn("_device_eligible")(self.q))

    @property
    def num_correlators(self):
        return int(self._fn("_get_num_correlators")(self.q))

    def templates(self):
        """the m x n template values as the library holds them"""
        p = np.zeros((self.num_correlators, self.n), np.complex64)
        self._fn("_get_templates")(self.q, ptr(p))
        return p

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def correlate(self, v):
        """one sample: None, or (tau_hat, dphi_hat, gamma_hat) at a detection"""
        e = np.zeros(3, np.float32)
        if self._fn("_correlate")(self.q, _by_value(v, CCCF), ptr(e[0:]), ptr(e[1:]), ptr(e[2:])):
            return e[0], e[1], e[2]
        return None

    @staticmethod
    def _outputs(max_det, index_dtype, guard):
        idx = np.full(max_det + guard, np.iinfo(index_dtype).max, index_dtype)
        est = [np.full(max_det + guard, np.float32(-77.0)) for _ in range(3)]
        return idx, est

    def correlate_block(self, x, max_det=64, guard=0):
        """host pointers; guard: extra entries left after max_det, returned
        untouched (for tests of max_det)"""
        x = _samples(x, CCCF)
        idx, est = self._outputs(max_det, np.uint32, guard)
        cnt = int(self._fn("_correlate_block")(self.q, ptr(x), len(x), ptr(idx), ptr(est[0]), ptr(est[1]),
                                               ptr(est[2]), max_det))
        k = len(idx) if guard else min(cnt, max_det)
        return cnt, idx[:k], est[0][:k], est[1][:k], est[2][:k]

    def correlate_block_dev(self, dx, n, drxy=0, max_det=64):
        """dx: n samples in device memory; drxy: 0 or n * m floats in device
        memory.  Waits for the object's stream."""
        idx, est = self._outputs(max_det, np.uint64, 0)
        cnt = int(self._fn("_correlate_block_dev")(self.q, dx, n, drxy or None, ptr(idx), ptr(est[0]), ptr(est[1]),
                                                   ptr(est[2]), max_det))
        k = min(cnt, max_det)
        return cnt, idx[:k], est[0][:k], est[1][:k], est[2][:k]


QDETECTOR_ROUTES = ("composed", "fused")
QDETECTOR_RECORD = np.dtype([("peak", np.float32), ("index", np.uint32), ("offset", np.int32),
                             ("energy", np.float32)])


def qdetector_route(nfft, rng=0, num_windows=1):
    """The seek kernel a qdetector launch takes (liquid_mi355x_qdetector_route)."""
    return QDETECTOR_ROUTES[lib().liquid_mi355x_qdetector_route(int(nfft), int(rng), int(num_windows))]


def set_qdetector_chunk(windows):
    """Seek windows per launch chunk of the qdetector (0: the default).  For tests."""
    lib().liquid_mi355x_qdetector_set_chunk(int(windows))


def set_qdetector_route(route):
    """"composed": every size's later launches take the composed path (and
    qdetector_route says so); None: the default.  For measurements."""
    lib().liquid_mi355x_qdetector_set_route(-1 if route is None else QDETECTOR_ROUTES.index(route))


def qdetector_chunk(nfft):
    return int(lib().liquid_mi355x_qdetector_chunk(int(nfft)))


class QDetector(_Obj):
    """qdetector_cccf: FFT preamble detector with a carrier sweep.  s: the
    template samples, or with linear=(ftype, k, m, beta) the symbols of
    create_linear.  execute(v) returns None or the nfft aligned samples;
    the block calls return a dict: count, idx, tau, gamma, dphi, phi (arrays
    of min(count, max_det)), frames (host call with frames=True), records
    (host call: a QDETECTOR_RECORD array) and num_records."""
    prefix = "qdetector_cccf"

    def __init__(self, s, linear=None):
        s = _samples(s, CCCF)
        if linear is None:
            self.q = self._fn("_create")(ptr(s), len(s))
        else:
            ftype, k, m, beta = linear
            code = LIQUID_FIRFILT[ftype] if isinstance(ftype, str) else int(ftype)
            self.q = self._fn("_create_linear")(ptr(s), len(s), code, k, m, float(beta))
        self.nfft = int(self._fn("_get_buf_len")(self.q))
        self.s_len = int(self._fn("_get_seq_len")(self.q))

    def sequence(self):
        p = self._fn("_get_sequence")(self.q)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (2 * self.s_len,)).view(np.complex64).copy()

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def set_threshold(self, v):
        self._fn("_set_threshold")(self.q, float(v))

    def set_range(self, v):
        self._fn("_set_range")(self.q, float(v))

    @property
    def threshold(self):
        return float(self._fn("_get_threshold")(self.q))

    @property
    def range(self):
        return int(self._fn("_get_range")(self.q))

    def estimates(self):
        """(tau_hat, gamma_hat, dphi_hat, phi_hat) of the last frame, float32"""
        return tuple(np.float32(self._fn(n)(self.q)) for n in ("_get_tau", "_get_gamma", "_get_dphi", "_get_phi"))

    def execute(self, v):
        p = self._fn("_execute")(self.q, _by_value(v, CCCF))
        if not p:
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (2 * self.nfft,)).view(np.complex64).copy()

    def _call(self, name, x, n, max_det, frames, records):
        idx = np.full(max_det, np.iinfo(np.uint64).max, np.uint64)
        est = [np.full(max_det, np.float32(-77.0)) for _ in range(4)]
        nrec = C.c_ulonglong(0)
        cnt = int(self._fn(name)(self.q, x, n, max_det, ptr(idx), ptr(est[0]), ptr(est[1]), ptr(est[2]), ptr(est[3]),
                                 frames, records, C.cast(C.byref(nrec), C.c_void_p)))
        k = min(cnt, max_det)
        return {"count": cnt, "idx": idx[:k], "tau": est[0][:k], "gamma": est[1][:k], "dphi": est[2][:k],
                "phi": est[3][:k], "num_records": int(nrec.value)}

    def execute_block(self, x, max_det=16, frames=False, records=True):
        """host pointers"""
        x = _samples(x, CCCF)
        fr = np.zeros((max_det, self.nfft), np.complex64) if frames else None
        rec = np.zeros(1 + (len(x) + self.nfft) // (self.nfft // 2), QDETECTOR_RECORD) if records else None
        r = self._call("_execute_block", ptr(x), len(x), max_det, None if fr is None else ptr(fr),
                       None if rec is None else ptr(rec))
        if fr is not None:
            r["frames"] = fr[:len(r["idx"])]
        if rec is not None:
            r["records"] = rec[:r["num_records"]]
        return r

    def execute_block_dev(self, dx, n, max_det=16, dframes=0, drecords=0):
        """dx: n samples in device memory; dframes / drecords: 0 or device
        memory.  Waits for the object's stream."""
        return self._call("_execute_block_dev", dx, n, max_det, dframes or None, drecords or None)


LIQUID_NCO, LIQUID_VCO = 0, 1


class NCO(_Obj):
    """nco_crcf: oscillator, PLL and mixer; typ LIQUID_NCO (sine table) or
    LIQUID_VCO (sinf / cosf).  The per-sample calls run on the host (the
    constructor needs no GPU); mix_block_up / mix_block_down run on the GPU when
    device_eligible, else in the library's host loop.  plan="direct" or
    "periodic" forces the form of the phase plan (LQ_NCO_PLAN, for tests)."""
    prefix = "nco_crcf"
    TILE = _LibConst("liquid_mi355x_nco_tile")               # samples per workgroup
    CHECKPOINT = _LibConst("liquid_mi355x_nco_checkpoint")   # positions per checkpoint of the plan

    def __init__(self, typ=LIQUID_NCO, plan=None):
        assert typ in (LIQUID_NCO, LIQUID_VCO) and plan in (None, "direct", "periodic")
        self.type = typ
        old = os.environ.get("LQ_NCO_PLAN")
        try:
            os.environ.pop("LQ_NCO_PLAN", None)
            if plan:
                os.environ["LQ_NCO_PLAN"] = plan
            self.q = self._fn("_create")(typ)
        finally:
            os.environ.pop("LQ_NCO_PLAN", None)
            if old is not None:
                os.environ["LQ_NCO_PLAN"] = old

    @property
    def device_eligible(self):
        return bool(self._fn("_device_eligible")(self.q))

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_frequency(self):
        return np.float32(self._fn("_get_frequency")(self.q))

    def set_frequency(self, v):
        self._fn("_set_frequency")(self.q, float(v))

    def adjust_frequency(self, v):
        self._fn("_adjust_frequency")(self.q, float(v))

    def get_phase(self):
        return np.float32(self._fn("_get_phase")(self.q))

    def set_phase(self, v):
        self._fn("_set_phase")(self.q, float(v))

    def adjust_phase(self, v):
        self._fn("_adjust_phase")(self.q, float(v))

    def step(self):
        self._fn("_step")(self.q)

    def sin(self):
        return np.float32(self._fn("_sin")(self.q))

    def cos(self):
        return np.float32(self._fn("_cos")(self.q))

    def sincos(self):
        s, c = C.c_float(), C.c_float()
        self._fn("_sincos")(self.q, C.byref(s), C.byref(c))
        return np.float32(s.value), np.float32(c.value)

    def cexpf(self):
        y = np.zeros(1, np.complex64)
        self._fn("_cexpf")(self.q, ptr(y))
        return y[0]

    def pll_set_bandwidth(self, bw):
        self._fn("_pll_set_bandwidth")(self.q, float(bw))

    def pll_step(self, dphi):
        self._fn("_pll_step")(self.q, float(dphi))

    def mix_up(self, v):
        y = np.zeros(1, np.complex64)
        self._fn("_mix_up")(self.q, _by_value(v, CRCF), ptr(y))
        return y[0]

    def mix_down(self, v):
        y = np.zeros(1, np.complex64)
        self._fn("_mix_down")(self.q, _by_value(v, CRCF), ptr(y))
        return y[0]

    def _block(self, name, x, n, y, inplace):
        if isinstance(x, DeviceBuffer):
            n = x.nbytes // 8 if n is None else n
            self._fn(name + "_dev")(self.q, x.p, (x if y is None else y).p, n)
            return x if y is None else y
        x = _samples(x, CRCF)
        y = x.copy() if inplace else np.zeros(len(x), np.complex64)
        self._fn(name)(self.q, ptr(y) if inplace else ptr(x), ptr(y), len(x))
        return y

    def mix_block_up(self, x, n=None, y=None, inplace=False):
        """y = x exp(+j theta), stepping.  x a numpy array (returns the output
        array; inplace: the library writes over its input array) or a
        DeviceBuffer (n samples, default all of it, into DeviceBuffer y,
        default x itself; stream-ordered: synchronize() before reading)."""
        return self._block("_mix_block_up", x, n, y, inplace)

    def mix_block_down(self, x, n=None, y=None, inplace=False):
        return self._block("_mix_block_down", x, n, y, inplace)

    def mix_block_up_dev(self, dx, dy, n):
        self._fn("_mix_block_up_dev")(self.q, dx, dy, n)

    def mix_block_down_dev(self, dx, dy, n):
        self._fn("_mix_block_down_dev")(self.q, dx, dy, n)


def nco_walk(typ, theta0, d_theta, n, periodic):
    """liquid_mi355x_nco_walk: (theta, index, pre-period, period) of the plan
    from (theta0, d_theta) for positions 0 .. n-1, or None if there is no plan."""
    th, idx = np.zeros(n, np.float32), np.zeros(n, np.uint32)
    pre, per = ull(0), ull(0)
    r = lib().liquid_mi355x_nco_walk(typ, float(theta0), float(d_theta), n, 1 if periodic else 0, ptr(th), ptr(idx),
                                     C.byref(pre), C.byref(per))
    return None if r < 0 else (th, idx, pre.value, per.value)


def unwrap_phase(theta, advanced=False):
    t = np.array(theta, np.float32)
    (lib().liquid_unwrap_phase2 if advanced else lib().liquid_unwrap_phase)(ptr(t), len(t))
    return t


class FreqMod(_Obj):
    """freqmod: analog FM modulator, s[n] = table[phase >> 6], phase the sum of
    roundf(kf 2^16 m[k]) modulo 2^16.  modulate() runs on the host (the
    constructor needs no GPU); modulate_block runs on the GPU."""
    prefix = "freqmod"
    TILE = _LibConst("liquid_mi355x_freqmod_tile")            # samples per workgroup
    SCAN_PASS = _LibConst("liquid_mi355x_freqmod_scan_pass")  # tiles per pass of the scan across tile sums

    def __init__(self, kf):
        self.kf = float(kf)
        self.q = self._fn("_create")(self.kf)

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_phase(self):
        return int(self._fn("_get_phase")(self.q))

    def get_table(self):
        t = np.zeros(1024, np.complex64)
        self._fn("_get_table")(self.q, ptr(t))
        return t

    def modulate(self, m):
        s = np.zeros(1, np.complex64)
        self._fn("_modulate")(self.q, float(m), ptr(s))
        return s[0]

    def modulate_block(self, m, n=None, s=None):
        """m a numpy array (returns the output array) or a DeviceBuffer (n
        samples, default all of it, into DeviceBuffer s; stream-ordered:
        synchronize() before reading)"""
        if isinstance(m, DeviceBuffer):
            n = m.nbytes // 4 if n is None else n
            self._fn("_modulate_block_dev")(self.q, m.p, n, s.p)
            return s
        m = np.ascontiguousarray(m, np.float32)
        s = np.zeros(len(m), np.complex64)
        self._fn("_modulate_block")(self.q, ptr(m), len(m), ptr(s))
        return s

    def modulate_block_dev(self, dm, n, ds):
        self._fn("_modulate_block_dev")(self.q, dm, n, ds)


class FreqDem(_Obj):
    """freqdem: analog FM demodulator, m[n] = arg(conj(r[n-channels]) r[n]) /
    (2 pi kf); channels > 1 demodulates interleaved channels (a channelizer's
    frame-major output).  demodulate() runs on the host (the constructor needs
    no GPU); demodulate_block runs on the GPU."""
    prefix = "freqdem"
    TILE = _LibConst("liquid_mi355x_freqdem_tile")       # samples per workgroup (channels < SWITCH)
    SWITCH = _LibConst("liquid_mi355x_freqdem_switch")   # channels from which a lane walks its own channel
    FRAMES = _LibConst("liquid_mi355x_freqdem_frames")   # frames of one such walk

    def __init__(self, kf, channels=1):
        self.kf, self.channels = float(kf), int(channels)
        self.q = self._fn("_create")(self.kf) if self.channels == 1 else \
            self._fn("_create_channels")(self.kf, self.channels)

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def get_channels(self):
        return int(self._fn("_get_channels")(self.q))

    def demodulate(self, r):
        m = np.zeros(1, np.float32)
        self._fn("_demodulate")(self.q, _by_value(r, CRCF), ptr(m))
        return m[0]

    def demodulate_block(self, r, n=None, m=None):
        """r a numpy array (returns the output array) or a DeviceBuffer (n
        samples, default all of it, into DeviceBuffer m; stream-ordered:
        synchronize() before reading)"""
        if isinstance(r, DeviceBuffer):
            n = r.nbytes // 8 if n is None else n
            self._fn("_demodulate_block_dev")(self.q, r.p, n, m.p)
            return m
        r = _samples(r, CRCF)
        m = np.zeros(len(r), np.float32)
        self._fn("_demodulate_block")(self.q, ptr(r), len(r), ptr(m))
        return m

    def demodulate_block_dev(self, dr, n, dm):
        self._fn("_demodulate_block_dev")(self.q, dr, n, dm)


IIRDES_FILTERTYPES = {"butter": 0, "cheby1": 1, "cheby2": 2, "ellip": 3, "bessel": 4}
IIRDES_BANDTYPES = {"lowpass": 0, "highpass": 1, "bandpass": 2, "bandstop": 3}
IIRDES_FORMATS = {"sos": 0, "tf": 1}


def _iirdes_codes(ftype, btype, fmt):
    return (IIRDES_FILTERTYPES[ftype] if isinstance(ftype, str) else int(ftype),
            IIRDES_BANDTYPES[btype] if isinstance(btype, str) else int(btype),
            IIRDES_FORMATS[fmt] if isinstance(fmt, str) else int(fmt))


class _IirRate(_Obj):
    """iirdecim_<t> / iirinterp_<t>: IirDecim(t, M, b, a) is create; the
    classmethods default(t, M, order) and prototype(t, M, ...) are the other
    constructors.  Host arrays through execute / execute_block, device
    pointers through execute_block_dev (n counted as for execute_block)."""

    def __init__(self, t, M, b, a):
        self.t, self.M = t, int(M)
        self.prefix = self.family % t
        self._b, self._a = _coefs(b, t), _coefs(a, t)
        self.q = self._fn("_create")(self.M, ptr(self._b), len(self._b), ptr(self._a), len(self._a))

    @classmethod
    def default(cls, t, M, order):
        return cls.construct("_create_default", (M, order), t=t, M=int(M))

    @classmethod
    def prototype(cls, t, M, ftype, btype, fmt, order, fc, f0=0.0, Ap=0.1, As=60.0):
        return cls.construct("_create_prototype", (M,) + _iirdes_codes(ftype, btype, fmt) + (order, fc, f0, Ap, As),
                             t=t, M=int(M))

    @property
    def device_eligible(self):
        return bool(self._fn("_device_eligible")(self.q))

    def reset(self):
        self._fn("_reset")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def groupdelay(self, fc):
        return float(self._fn("_groupdelay")(self.q, fc))

    def execute_block_dev(self, dx, n, dy):
        self._fn("_execute_block_dev")(self.q, dx, n, dy)


class IirDecim(_IirRate):
    family = "iirdecim_%s"

    def execute(self, x):
        """M samples -> one"""
        x = _samples(x, self.t)
        assert len(x) == self.M
        y = np.zeros(1, _out_dtype(self.t))
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y[0]

    def execute_block(self, x):
        """n M samples -> n"""
        x = _samples(x, self.t)
        assert len(x) % self.M == 0
        y = np.zeros(len(x) // self.M, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), len(y), ptr(y))
        return y


class IirInterp(_IirRate):
    family = "iirinterp_%s"

    def execute(self, v):
        """one sample -> M"""
        y = np.zeros(self.M, _out_dtype(self.t))
        self._fn("_execute")(self.q, _by_value(v, self.t), ptr(y))
        return y

    def execute_block(self, x):
        """n samples -> n M"""
        x = _samples(x, self.t)
        y = np.zeros(len(x) * self.M, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), len(x), ptr(y))
        return y


def iirdes(ftype, btype, fmt, order, fc, f0=0.0, Ap=0.1, As=60.0):
    """liquid_iirdes -> (B, A): 3 coefficients per section (sos) or N + 1
    each (tf), N the order, doubled for band-pass and band-stop"""
    ft, bt, fm = _iirdes_codes(ftype, btype, fmt)
    N = 2 * order if bt >= 2 else order
    n = 3 * ((N + 1) // 2) if fm == 0 else N + 1
    B, A = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib().liquid_iirdes(ft, bt, fm, order, fc, f0, Ap, As, ptr(B), ptr(A))
    return B, A


def _azpk(fn, n, nz, *args):
    z, p, k = np.zeros(max(nz, 1), np.complex64), np.zeros(n, np.complex64), np.zeros(1, np.complex64)
    getattr(lib(), fn)(n, *args, ptr(z), ptr(p), ptr(k))
    return z[:nz], p, complex(k[0])


def butter_azpkf(n):
    """-> (zeros, poles, gain) of the analog prototype"""
    return _azpk("butter_azpkf", n, 0)


def cheby1_azpkf(n, ep):
    return _azpk("cheby1_azpkf", n, 0, ep)


def cheby2_azpkf(n, es):
    return _azpk("cheby2_azpkf", n, 2 * (n // 2), es)


def ellip_azpkf(n, ep, es):
    return _azpk("ellip_azpkf", n, 2 * (n // 2), ep, es)


def bessel_azpkf(n):
    return _azpk("bessel_azpkf", n, 0)


def bilinear_zpkf(za, pa, ka, m):
    """-> (zd, pd, kd), len(pa) each"""
    za, pa = np.ascontiguousarray(za, np.complex64), np.ascontiguousarray(pa, np.complex64)
    zd, pd, kd = np.zeros(len(pa), np.complex64), np.zeros(len(pa), np.complex64), np.zeros(1, np.complex64)
    zin = za if len(za) else np.zeros(1, np.complex64)
    lib().bilinear_zpkf(ptr(zin), len(za), ptr(pa), len(pa), cfloat(float(np.real(ka)), float(np.imag(ka))), m,
                        ptr(zd), ptr(pd), ptr(kd))
    return zd, pd, complex(kd[0])


def iirdes_isstable(b, a):
    b, a = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(a, np.float32)
    assert len(b) == len(a)
    return bool(lib().iirdes_isstable(ptr(b), ptr(a), len(a)))


def liquid_cplxpair(z, tol):
    z = np.ascontiguousarray(z, np.complex64)
    p = np.zeros(len(z), np.complex64)
    lib().liquid_cplxpair(ptr(z), len(z), tol, ptr(p))
    return p


def iirdes_pll_active_lag(w, zeta, K):
    b, a = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib().iirdes_pll_active_lag(w, zeta, K, ptr(b), ptr(a))
    return b, a


def iirdes_pll_active_PI(w, zeta, K):
    b, a = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib().iirdes_pll_active_PI(w, zeta, K, ptr(b), ptr(a))
    return b, a


def iirdes_dzpk2sosf(z, p, k):
    """zeros, poles, gain -> (B, A), 3 coefficients per section"""
    z, p = np.ascontiguousarray(z, np.complex64), np.ascontiguousarray(p, np.complex64)
    assert len(z) == len(p)
    ns = (len(z) + 1) // 2
    B, A = np.zeros(3 * ns, np.float32), np.zeros(3 * ns, np.float32)
    lib().iirdes_dzpk2sosf(ptr(z), ptr(p), len(z), cfloat(float(np.real(k)), float(np.imag(k))), ptr(B), ptr(A))
    return B, A


def iir_group_delay(b, a, fc):
    b, a = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(a, np.float32)
    return float(lib().iir_group_delay(ptr(b), len(b), ptr(a), len(a), fc))


class MsResamp2(_Obj):
    family = "msresamp2_%s"

    def __init__(self, typ, ns, fc, f0, As, t=CRCF):
        self.t, self.typ, self.M = t, typ, 1 << ns
        self.prefix = self.family % t
        self.q = self._fn("_create")(typ, ns, fc, f0, As)

    def reset(self):
        self._fn("_reset")(self.q)

    def execute_block_dev(self, dx, n, dy):
        """n calls (n inputs when interpolating, n M when decimating) on device pointers."""
        self._fn("_execute_block_dev")(self.q, dx, n, dy)

    def synchronize(self):
        self._fn("_synchronize")(self.q)

    def execute_block(self, x):
        x = _samples(x, self.t)
        n = len(x) if self.typ == LIQUID_RESAMP_INTERP else len(x) // self.M
        y = np.zeros(n * self.M if self.typ == LIQUID_RESAMP_INTERP else n, _out_dtype(self.t))
        self._fn("_execute_block")(self.q, ptr(x), n, ptr(y))
        return y

    def execute(self, x):
        x = _samples(x, self.t)
        y = np.zeros(self.M if self.typ == LIQUID_RESAMP_INTERP else 1, _out_dtype(self.t))
        self._fn("_execute")(self.q, ptr(x), ptr(y))
        return y

    def get_delay(self):
        return self._fn("_get_delay")(self.q)


class MsResamp(_Obj):
    family = "msresamp_%s"

    def __init__(self, rate, As, t=CRCF):
        self.t = t
        self.prefix = self.family % t
        self.q = self._fn("_create")(rate, As)

    def reset(self):
        self._fn("_reset")(self.q)

    def num_output(self, nx):
        return int(self._fn("_num_output")(self.q, nx))

    def execute(self, x):
        x = _samples(x, self.t)
        y = np.zeros(max(1, self.num_output(len(x))), _out_dtype(self.t))
        ny = C.c_uint(0)
        self._fn("_execute")(self.q, ptr(x), len(x), ptr(y), C.byref(ny))
        return y[:ny.value]

    def execute_block_dev(self, dx, nx, dy):
        ny = C.c_ulonglong(0)
        self._fn("_execute_block_dev")(self.q, dx, nx, dy, C.byref(ny))
        return ny.value

    def get_delay(self):
        return self._fn("_get_delay")(self.q)

    def synchronize(self):
        self._fn("_synchronize")(self.q)


# ------------------------------------------------------------------ FFT plan API (liquid.h:1113-1216)
def fft_run(x, direction=+1):
    x = np.ascontiguousarray(x, np.complex64)
    y = np.zeros_like(x)
    lib().fft_run(len(x), ptr(x), ptr(y), direction, 0)
    return y


def fft_r2r(x, typ):
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    lib().fft_r2r_1d_run(len(x), ptr(x), ptr(y), typ, 0)
    return y


def fft_batch(X, direction=+1):
    """fft_execute_batch over the rows of X (host arrays)."""
    X = np.ascontiguousarray(X, np.complex64)
    b, n = X.shape
    Y = np.zeros_like(X)
    p = lib().fft_create_plan(n, None, None, direction, 0)
    try:
        lib().fft_execute_batch(p, ptr(X), ptr(Y), b)
    finally:
        lib().fft_destroy_plan(p)
    return Y


def fft_shift(x):
    x = np.array(x, np.complex64)
    lib().fft_shift(ptr(x), len(x))
    return x



# ------------------------------------------------------------------ spectral periodogram (liquid.h:1220-1290)
class Spgram(_Obj):
    def __init__(self, nfft, window=None, real_in=False, default=False, kaiser=None):
        self.nfft, self.real_in = nfft, real_in
        self.prefix = "spgramf" if real_in else "spgramcf"
        if default:
            self.q = self._fn("_create_default")(nfft)
        elif kaiser is not None:               # (window_len, beta)
            self.q = self._fn("_create_kaiser")(nfft, kaiser[0], kaiser[1])
        else:
            self._w = np.ascontiguousarray(window, np.float32)
            self.q = self._fn("_create")(nfft, ptr(self._w), len(self._w))

    def _x(self, x):
        return np.ascontiguousarray(x, np.float32 if self.real_in else np.complex64)

    def reset(self):
        self._fn("_reset")(self.q)

    def push(self, v):
        self._fn("_push")(self.q, float(np.real(v)) if self.real_in else _by_value(v, CRCF))

    def write(self, x):
        x = self._x(x)
        self._fn("_write")(self.q, ptr(x), len(x))

    def execute(self):
        X = np.zeros(self.nfft, np.complex64)
        self._fn("_execute")(self.q, ptr(X))
        return X

    def execute_psd(self):
        X = np.zeros(self.nfft, np.float32)
        self._fn("_execute_psd")(self.q, ptr(X))
        return X

    def accumulate_psd(self, x, alpha):
        x = self._x(x)
        self._fn("_accumulate_psd")(self.q, ptr(x), alpha, len(x))

    def write_accumulation(self):
        X = np.zeros(self.nfft, np.float32)
        self._fn("_write_accumulation")(self.q, ptr(X))
        return X

    def estimate_psd(self, x):
        x = self._x(x)
        X = np.zeros(self.nfft, np.float32)
        self._fn("_estimate_psd")(self.q, ptr(x), len(x), ptr(X))
        return X

    def accumulate_psd_dev(self, dx, n, alpha):
        """n samples at the device address dx"""
        self._fn("_accumulate_psd_dev")(self.q, dx, alpha, n)

    def estimate_psd_dev(self, dx, n, dpsd):
        """n samples at the device address dx; nfft floats (dB, shifted) to the device address dpsd"""
        self._fn("_estimate_psd_dev")(self.q, dx, n, dpsd)

    def synchronize(self):
        self._fn("_synchronize")(self.q)
