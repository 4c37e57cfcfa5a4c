"""Tensor-level wrappers over the C ABI (include/footprints_hip.h).

Every function takes contiguous float32 CUDA tensors, launches on torch's
current stream and returns immediately (async).  PyTorch only owns memory and
streams here; there is no torch compute op and no fallback in this module.
"""
import ctypes as C

import os

import torch

from . import _lib
from ._lib import ConvDesc

_workspaces = {}
# allocation generation: bumped whenever a buffer that kernels address by raw pointer is (re)allocated -- the activation arena
# (Engine.buf), a workspace below, the flat parameter / gradient buffers, the pack tables.  A recorded launch plan freezes raw
# pointers; TrainStep compares the generation it recorded at with the current one and drops its plans on a mismatch.
_alloc_gen = [0]


def alloc_generation():
    return _alloc_gen[0]


def bump_alloc_generation():
    _alloc_gen[0] += 1
_NO_SPLITK = bool(int(__import__("os").environ.get("FP_NO_SPLITK", "0")))   # debugging aid: never split small grids along K


def _chk(t, name="tensor"):
    if t is None:
        return 0
    if not (t.is_cuda and t.is_contiguous()):
        raise RuntimeError("footprints_amd.ops: %s must be a contiguous CUDA tensor (no CPU path in the product)" % name)
    return t.data_ptr()


def _f32(t, name="tensor"):
    if t is not None and t.dtype != torch.float32:
        raise RuntimeError("footprints_amd.ops: %s must be float32" % name)
    return _chk(t, name)


_cur_stream = None      # (torch stream, raw handle) while inside on_stream(): saves ~900 torch.cuda.current_stream() calls per step


def stream():
    return _cur_stream[1] if _cur_stream is not None else torch.cuda.current_stream().cuda_stream


class on_stream:
    """`with torch.cuda.stream(s)` that also caches the raw handle for the launch wrappers of this module"""

    def __init__(self, s):
        self.s = s
        self.ctx = torch.cuda.stream(s)

    def __enter__(self):
        global _cur_stream
        self.prev = _cur_stream
        self.ctx.__enter__()
        _cur_stream = (self.s, self.s.cuda_stream)
        return self.s

    def __exit__(self, *exc):
        global _cur_stream
        _cur_stream = self.prev
        return self.ctx.__exit__(*exc)


def current_stream():
    return _cur_stream[0] if _cur_stream is not None else torch.cuda.current_stream()


def event_record(stream_obj=None):
    """record a library event on `stream_obj` (default: the current launch stream) -> event id for event_wait"""
    h = stream_obj.cuda_stream if stream_obj is not None else stream()
    ev = _lib.load().fp_event_record(h)
    if ev < 0:
        raise RuntimeError("fp_event_record: %s" % _lib.load().fp_last_error_string().decode())
    return ev


def event_wait(stream_obj, ev):
    _lib.check(_lib.load().fp_event_wait(stream_obj.cuda_stream, ev), "fp_event_wait")


def stream_wait_stream(consumer, producer):
    """everything queued on `producer` so far happens before whatever is queued on `consumer` from now on"""
    event_wait(consumer, event_record(producer))


_query_cache = {}


def _cached_query(fn, desc):
    """shape predicates / workspace sizes are pure functions of the descriptor: ask the library once per distinct shape"""
    key = (fn, bytes(desc))
    v = _query_cache.get(key)
    if v is None:
        v = _query_cache[key] = getattr(_lib.load(), fn)(C.byref(desc))
    return v


_RELEASE_SYNC = bool(int(os.environ.get("FP_RELEASE_SYNC", "1")))
_release_hooks = []      # test instrumentation (tests/test_gpu_lifetime.py): callables (old tensor, what) run whenever a buffer is let go


def release(old, what):
    """Every place that REPLACES a device buffer which earlier launches were handed (a workspace that grows, an arena buffer of the engine
    that is re-allocated) lets go of the old one through here.  Kernels that follow on the stream are ordered behind the launches that used
    it; what the HOST does next is not -- the caching allocator hands the block out again at once, and a small pageable host-to-device copy
    into it does not wait for kernels still writing there (round 5, profiles/round5_notes.md section 7: a split-K convolution's late partial
    sums landed on a pack-job table).  So: wait for the device first (start-up and shape changes only; never under stream capture, where the
    pool keeps captured blocks alive), then tell the hooks -- the lifetime stress test fills the old block with a sentinel on an idle stream
    and checks afterwards that nothing wrote into it (round 6, VERDICT r5 "Next" 9)."""
    if old is None:
        return
    if _RELEASE_SYNC and not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize(old.device)
    for hook in _release_hooks:
        hook(old, what)


def workspace(nbytes, device, tag="main"):
    """Grow-only scratch buffer per (device, stream, tag); a growth lets go of the old buffer through `release` (which says why it waits)."""
    # one scratch buffer per (device, stream, tag): kernels on concurrent streams must not share partials
    key = (device.index, stream(), tag)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        release(ws, "workspace:%s" % tag)
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
        bump_alloc_generation()
    return ws


def make_desc(N, OH, OW, IH, IW, C0, C1, Nout, K, stride, pad, gather, act=0, epi=0):
    return ConvDesc(N, OH, OW, IH, IW, C0, C1, Nout, K, K, stride, pad, gather, act, epi)


def _conv(fn, ws_query, desc, operands, y, bias, addend, addend_mask, actsrc, bn_out, slots=(), epi=0):
    """One forward / data-gradient convolution launch through entry point `fn`: a private copy of the descriptor with the epilogue flags
    of the optional arguments (and `epi`), the split-K workspace `ws_query` asks for (None: none is passed), the call, the check.
    `operands` / `slots`: the entry point's pointers in front of `bias` / behind the workspace."""
    d = ConvDesc.from_buffer_copy(desc)
    d.epi = desc.epi | epi | (_lib.EPI_BIAS if bias is not None else 0) | (_lib.EPI_ADDEND if addend is not None else 0) | \
        (_lib.EPI_ADDEND_MASK if addend_mask is not None else 0)
    need = _cached_query(ws_query, d) if ws_query else 0
    ws_ptr, ws_n = 0, 0
    if need > 0:
        ws = workspace(need, y.device, "igemm")
        ws_ptr, ws_n = ws.data_ptr(), ws.numel()
    _lib.check(getattr(_lib.load(), fn)(C.byref(d), *operands, _f32(bias), _f32(addend), _f32(addend_mask), _f32(actsrc), _f32(y, "y"), ws_ptr, ws_n,
                                        *slots, _aux(bn_out=bn_out), stream()), fn)
    return y


# The one difference between the two families: the flattened kernels split only when they are handed a workspace, so FP_NO_SPLITK is
# honoured by passing none; the tile plan decides the split from the shape alone and requires its workspace, so it is always passed.
_IGEMM_WS = None if _NO_SPLITK else "fp_conv_igemm_workspace"
_TILE_WS = "fp_conv3x3_bf3_workspace"


def conv_igemm(desc, src0, src1, wpacked, y, bias=None, addend=None, addend_mask=None, actsrc=None, bn_out=None):
    return _conv("fp_conv_igemm", _IGEMM_WS, desc, (_f32(src0, "src0"), _f32(src1, "src1"), _f32(wpacked, "wpacked")), y, bias, addend, addend_mask,
                 actsrc, bn_out)


def conv_stem_hp_supported(desc):
    return bool(_cached_query("fp_conv_stem_hp_supported", desc))


def conv_stem_hp(desc, img, wpacked_hp, y, amax_w, bias=None, amax_out=None, bn_out=None):
    """the 7x7 / 2 stem on the NCHW image with fp16-pair operands (weights from a PACK_STEM_HP job); optional side outputs: amax_out, bn_out"""
    d = ConvDesc.from_buffer_copy(desc)
    if bias is not None:
        d.epi |= _lib.EPI_BIAS
    _lib.check(_lib.load().fp_conv_stem_hp(C.byref(d), _f32(img), _f32(wpacked_hp), _f32(bias), _f32(y), _u32(amax_w, "amax_w"),
                                           _aux(amax_out, bn_out), stream()),
               "fp_conv_stem_hp")
    return y


def conv_stem_wgrad_hp(desc, img, dz, dw, amax_dz, accumulate=False):
    lib = _lib.load()
    ws = workspace(_cached_query("fp_conv_wgrad_workspace", desc), dz.device)
    _lib.check(lib.fp_conv_stem_wgrad_hp(C.byref(desc), _f32(img), _f32(dz), _f32(dw), int(bool(accumulate)), ws.data_ptr(), ws.numel(),
                                         _u32(amax_dz, "amax_dz"), stream()), "fp_conv_stem_wgrad_hp")
    return dw


def conv_igemm_hp_supported(desc):
    return bool(_cached_query("fp_conv_igemm_hp_supported", desc))


def conv_igemm_hp(desc, src, wpacked_hp, y, amax_src, amax_w, bias=None, addend=None, addend_mask=None, actsrc=None, bn_out=None):
    """flattened implicit GEMM with fp16-pair operands (3x3 stride 2, 1x1, their data gradients): weights from FP_PACK_{FWD,DGRAD}_HP"""
    return _conv("fp_conv_igemm_hp", _IGEMM_WS, desc, (_f32(src, "src"), _chk(wpacked_hp, "wpacked_hp")), y, bias, addend, addend_mask, actsrc, bn_out,
                 slots=(_u32(amax_src), _u32(amax_w)))


def conv3x3_bf3_supported(desc):
    return bool(_cached_query("fp_conv3x3_bf3_supported", desc))


_bf16x2 = False      # opt-in inference mode of the bf16 tile kernel (Engine.forward sets it around an eval forward): two bf16 terms per operand


def conv3x3_bf3(desc, src, wpacked_bf3, y, bias=None, addend=None, addend_mask=None, actsrc=None, src1=None, bn_out=None):
    """3x3 stride-1 conv / data-gradient with exactly split bf16x3 operands (same semantics as conv_igemm; src1 = the skip tensor
    of the GATHER_FWD_REFLECT_UP2 concat)"""
    fwd = desc.gather in (_lib.GATHER_FWD_ZERO, _lib.GATHER_FWD_REFLECT, _lib.GATHER_FWD_REFLECT_UP2)
    return _conv("fp_conv3x3_bf3", _TILE_WS, desc, (_f32(src, "src"), _f32(src1, "src1"), _f32(wpacked_bf3, "wpacked")), y, bias, addend, addend_mask,
                 actsrc, bn_out, epi=_lib.EPI_BF16X2 if _bf16x2 and fwd else 0)


# ---- fp16-pair operands (include/footprints_hip.h "hp"): amax slots are int32 tensors of amax_elems() elements ---------------------
_amax_elems = None


def amax_elems():
    """int32 elements of storage per amax slot (FP_AMAX_ELEMS of the loaded library)"""
    global _amax_elems
    if _amax_elems is None:
        _amax_elems = int(_lib.load().fp_amax_slot_elems())
    return _amax_elems


def _u32(t, what="slot"):
    if t is None:
        return 0
    if t.dtype != torch.int32 or not t.is_cuda or t.numel() < amax_elems():
        raise RuntimeError("footprints_amd: %s must be a CUDA int32 tensor of >= %d elements" % (what, amax_elems()))
    return t.data_ptr()


class BnOut:
    """BatchNorm partials out of a convolution's epilogue (fp_aux.bn_* of include/footprints_hip.h): pass as `bn_out=` to the convolution
    call; afterwards `.nblk` = number of partial blocks the launch wrote (0 = it could not emit: run the BatchNorm's own reduction pass).
    Forward statistics (count, mean, M2) with z2d None; the backward sums (sum g, sum g * xhat) of the BatchNorm whose input z2d and saved
    statistics are given otherwise.  Round 6: an explicit argument of the launch -- rounds 3-5 armed a per-thread sink in the library."""

    def __init__(self, part, z2d=None, save_mean=None, save_invstd=None):
        self.part, self.z, self.mean, self.invstd = part, z2d, save_mean, save_invstd
        self._n = C.c_int32(0)

    @property
    def nblk(self):
        return int(self._n.value)


def _aux(amax_out=None, bn_out=None):
    """the `const fp_aux*` argument of one launch: None when there is nothing to ask for (the struct is read during the call only)"""
    if amax_out is None and bn_out is None:
        return None
    a = _lib.Aux()
    if amax_out is not None:
        a.amax_out = _u32(amax_out, "amax_out")
    if bn_out is not None:
        bn_out._n.value = 0
        a.bn_part, a.bn_capacity_floats, a.bn_nblk_out = _f32(bn_out.part, "part"), bn_out.part.numel(), C.pointer(bn_out._n)
        if bn_out.z is not None:
            a.bnb_z, a.bnb_mean, a.bnb_invstd = _f32(bn_out.z, "z"), _f32(bn_out.mean, "save_mean"), _f32(bn_out.invstd, "save_invstd")
    return C.byref(a)


def zero_u32(t):
    _lib.check(_lib.load().fp_zero_u32(t.data_ptr(), t.numel(), stream()), "fp_zero_u32")
    return t


def amax_f32(x, slot):
    """slot (zeroed by the caller) <- max |x| (bit pattern, spread over the sub-slots)"""
    _lib.check(_lib.load().fp_amax_f32(_f32(x, "x"), x.numel(), _u32(slot), stream()), "fp_amax_f32")
    return slot


def amax_value(slot):
    """host-side read of a slot (tests / debugging): the float it encodes"""
    return float(slot[:amax_elems()].max().view(torch.int32).cpu().view(torch.float32))


def weight_amax(w, slot):
    """slot <- max |w| (zeroes the slot first): the scale of every fp16-pair packing of this weight tensor"""
    _lib.check(_lib.load().fp_weight_amax(_f32(w), w.numel(), _u32(slot), stream()), "fp_weight_amax")
    return slot


def new_slot(device="cuda"):
    return torch.zeros(amax_elems(), dtype=torch.int32, device=device)


def packed_weight_elems_hp(Cout, Cin, K, for_dgrad=False):
    return int(_lib.load().fp_packed_weight_elems_hp(Cout, Cin, K, K, int(for_dgrad)))


def pack_conv_weight_hp(w, wp, slot, for_dgrad=False, amax_ready=False):
    Cout, Cin, KH, KW = w.shape
    _lib.check(_lib.load().fp_pack_conv_weight_hp(_f32(w), _f32(wp), Cout, Cin, KH, KW, int(for_dgrad), _u32(slot), int(amax_ready), stream()),
               "fp_pack_conv_weight_hp")
    return wp


def conv3x3_hp(desc, src, wpacked_hp, y, amax_src, amax_w, amax_out=None, bias=None, addend=None, addend_mask=None, actsrc=None, src1=None,
               amax_src1=None, bn_out=None):
    """conv3x3_bf3 with fp16-pair operands; amax_* are slots (see amax_f32); amax_out (zeroed by the caller) receives max |y|"""
    return _conv("fp_conv3x3_hp", _TILE_WS, desc, (_f32(src, "src"), _f32(src1, "src1"), _f32(wpacked_hp, "wpacked")), y, bias, addend, addend_mask,
                 actsrc, bn_out, slots=(_u32(amax_src, "amax_src"), _u32(amax_src1, "amax_src1"), _u32(amax_w, "amax_w"), _u32(amax_out, "amax_out")))


def conv_igemm_bf3(desc, src, wpacked_bf3, y, bias=None, addend=None, addend_mask=None, actsrc=None, bn_out=None):
    """flattened implicit GEMM with EXACTLY split bf16x3 operands (3x3 stride 2, 1x1, their data gradients; the default operand format):
    weights from FP_PACK_{FWD,DGRAD}_BF3; shapes as conv_igemm_hp_supported"""
    return _conv("fp_conv_igemm_bf3", _IGEMM_WS, desc, (_f32(src, "src"), _chk(wpacked_bf3, "wpacked_bf3")), y, bias, addend, addend_mask, actsrc, bn_out)


def packed_weight_elems_bf3(Cout, Cin, K, for_dgrad=False):
    return int(_lib.load().fp_packed_weight_elems_bf3(Cout, Cin, K, K, int(for_dgrad)))


def pack_conv_weight_bf3(w, wp, for_dgrad=False):
    Cout, Cin, KH, KW = w.shape
    _lib.check(_lib.load().fp_pack_conv_weight_bf3(_f32(w), _f32(wp), Cout, Cin, KH, KW, int(for_dgrad), stream()), "fp_pack_conv_weight_bf3")
    return wp


def conv_wgrad(desc, src0, src1, dz, dw, accumulate=False):
    lib = _lib.load()
    need = _cached_query("fp_conv_wgrad_workspace", desc)
    ws = workspace(need, dz.device)
    _lib.check(lib.fp_conv_wgrad(C.byref(desc), _f32(src0), _f32(src1), _f32(dz), _f32(dw), int(bool(accumulate)),
                                 ws.data_ptr(), ws.numel(), stream()), "fp_conv_wgrad")
    return dw


def conv_wgrad_bf3_supported(desc):
    return _cached_query("fp_conv_wgrad_bf3_workspace", desc) >= 0


def conv_wgrad_bf3(desc, x, dz, dw, k_begin=0, accumulate=False, db=None, amax=None):
    """3x3 stride-1 weight gradient with split operands, into dw[:, k_begin:k_begin + C0]; db (optional) receives the bias gradient
    (column sums of dz) from the same pass.  amax = (slot of x, slot of dz): scaled fp16 pairs (three products); None: the exact
    bf16x3 split (six)"""
    lib = _lib.load()
    need = _cached_query("fp_conv_wgrad_bf3_workspace", desc)
    if need < 0:
        raise RuntimeError("fp_conv_wgrad_bf3: shape not supported")
    ws = workspace(need, dz.device)
    if amax is not None:
        return conv_wgrad_hp(desc, x, dz, dw, amax[0], amax[1], k_begin, accumulate, db, ws)
    _lib.check(lib.fp_conv_wgrad_bf3(C.byref(desc), _f32(x), _f32(dz), _f32(dw), _f32(db), dw.shape[1], k_begin, int(bool(accumulate)),
                                     ws.data_ptr(), ws.numel(), stream()), "fp_conv_wgrad_bf3")
    return dw


def conv_wgrad_slice(desc, src0, src1, dz, dw, k_begin, accumulate=False):
    """weight gradient of the input-channel slice [k_begin, k_begin + C0 + C1) of the wider gradient dw [Nout][Cin][K][K]"""
    lib = _lib.load()
    ws = workspace(lib.fp_conv_wgrad_workspace(C.byref(desc)), dz.device)
    _lib.check(lib.fp_conv_wgrad_slice(C.byref(desc), _f32(src0), _f32(src1), _f32(dz), _f32(dw), dw.shape[1], k_begin,
                                       int(bool(accumulate)), ws.data_ptr(), ws.numel(), stream()), "fp_conv_wgrad_slice")
    return dw


def up2_phase_wgrad_supported(N, h, w, C0, Nout):
    return _lib.load().fp_conv_up2_phase_wgrad_workspace(N, h, w, C0, Nout) >= 0


def conv_wgrad_hp(desc, x, dz, dw, amax_x, amax_dz, k_begin=0, accumulate=False, db=None, ws=None):
    lib = _lib.load()
    if ws is None:
        ws = workspace(_cached_query("fp_conv_wgrad_bf3_workspace", desc), dz.device)
    _lib.check(lib.fp_conv_wgrad_hp(C.byref(desc), _f32(x), _f32(dz), _f32(dw), _f32(db), dw.shape[1], k_begin, int(bool(accumulate)),
                                    ws.data_ptr(), ws.numel(), _u32(amax_x, "amax_x"), _u32(amax_dz, "amax_dz"), stream()), "fp_conv_wgrad_hp")
    return dw


def conv_up2_phase_wgrad_hp(low, dz, dw, amax_low, amax_dz, k_begin=0, accumulate=False, db=None):
    lib = _lib.load()
    N, h, w, C0 = low.shape
    Nout = dz.shape[3]
    need = lib.fp_conv_up2_phase_wgrad_workspace(N, h, w, C0, Nout)
    if need < 0:
        raise RuntimeError("fp_conv_up2_phase_wgrad_hp: shape not supported")
    ws = workspace(need, dz.device)
    _lib.check(lib.fp_conv_up2_phase_wgrad_hp(_f32(low), _f32(dz), _f32(dw), _f32(db), N, h, w, C0, Nout, dw.shape[1], k_begin,
                                              int(bool(accumulate)), ws.data_ptr(), ws.numel(), _u32(amax_low, "amax_low"),
                                              _u32(amax_dz, "amax_dz"), stream()), "fp_conv_up2_phase_wgrad_hp")
    return dw


def conv_up2_phase_wgrad(low, dz, dw, k_begin=0, accumulate=False, bf3=False, db=None):
    """db (bf3 only): also produce the bias gradient (column sums of dz) from the same pass"""
    lib = _lib.load()
    if db is not None and not bf3:
        raise RuntimeError("conv_up2_phase_wgrad: the fused bias gradient needs the bf16x3 kernel")
    N, h, w, C0 = low.shape
    Nout = dz.shape[3]
    need = lib.fp_conv_up2_phase_wgrad_workspace(N, h, w, C0, Nout)
    if need < 0:
        raise RuntimeError("fp_conv_up2_phase_wgrad: shape not supported")
    ws = workspace(need, dz.device)
    tail = (N, h, w, C0, Nout, dw.shape[1], k_begin, int(bool(accumulate)), ws.data_ptr(), ws.numel(), stream())
    if bf3:
        _lib.check(lib.fp_conv_up2_phase_wgrad_bf3(_f32(low), _f32(dz), _f32(dw), _f32(db), *tail), "fp_conv_up2_phase_wgrad_bf3")
    else:
        _lib.check(lib.fp_conv_up2_phase_wgrad(_f32(low), _f32(dz), _f32(dw), *tail), "fp_conv_up2_phase_wgrad")
    return dw


def packed_weight_elems(Cout, Cin, K, for_dgrad=False, stem=False):
    return int(_lib.load().fp_packed_weight_elems(Cout, Cin, K, K, int(for_dgrad), int(stem)))


def pack_conv_weight(w, wp, stem=False):
    Cout, Cin, KH, KW = w.shape
    _lib.check(_lib.load().fp_pack_conv_weight(_f32(w), _f32(wp), Cout, Cin, KH, KW, int(stem), stream()), "fp_pack_conv_weight")
    return wp


def pack_conv_weight_dgrad(w, wp):
    Cout, Cin, KH, KW = w.shape
    _lib.check(_lib.load().fp_pack_conv_weight_dgrad(_f32(w), _f32(wp), Cout, Cin, KH, KW, stream()), "fp_pack_conv_weight_dgrad")
    return wp


def up2_packed_weight_elems(Cout, c_count):
    return _lib.load().fp_up2_packed_weight_elems(Cout, c_count)


def pack_up2_weight(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_up2_weight(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()), "fp_pack_up2_weight")
    return wp


def pack_conv_weight_slice(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_conv_weight_slice(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()), "fp_pack_conv_weight_slice")
    return wp


def pack_up2_weight_bf3(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_up2_weight_bf3(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()), "fp_pack_up2_weight_bf3")
    return wp


def conv_up2_phase_fwd_hp(low, wphase_hp, bias, y, amax_low, amax_w, amax_out=None, act=0, addend=None):
    N, h, w, C0 = low.shape
    _lib.check(_lib.load().fp_conv_up2_phase_fwd_hp(_f32(low), _f32(wphase_hp), _f32(bias), _f32(addend), _f32(y), N, h, w, C0, y.shape[3],
                                                    int(act), _u32(amax_low, "amax_low"), _u32(amax_w, "amax_w"), _u32(amax_out, "amax_out"),
                                                    stream()), "fp_conv_up2_phase_fwd_hp")
    return y


def conv_up2_phase_dgrad_hp(dz, wpacked_hp, ext, amax_dz, amax_w):
    N, H2, W2, Cout = dz.shape
    _lib.check(_lib.load().fp_conv_up2_phase_dgrad_hp(_f32(dz), _f32(wpacked_hp), _f32(ext), N, H2 // 2, W2 // 2, Cout, ext.shape[3],
                                                      _u32(amax_dz, "amax_dz"), _u32(amax_w, "amax_w"), stream()), "fp_conv_up2_phase_dgrad_hp")
    return ext


def conv_up2_phase_fwd_bf3(low, wphase_bf3, bias, y, act=0, addend=None, amax_out=None):
    N, h, w, C0 = low.shape
    _lib.check(_lib.load().fp_conv_up2_phase_fwd_bf3(_f32(low), _f32(wphase_bf3), _f32(bias), _f32(addend), _f32(y), N, h, w, C0, y.shape[3],
                                                     int(act), _aux(amax_out), stream()), "fp_conv_up2_phase_fwd_bf3")
    return y


def pack_up2_weight_dgrad_bf3(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_up2_weight_dgrad_bf3(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()),
               "fp_pack_up2_weight_dgrad_bf3")
    return wp


def conv_up2_phase_dgrad_bf3(dz, wpacked_bf3, ext):
    """gradient wrt the low-res input of an upsample conv on the (h+2) x (w+2) extended grid (up2_fold_bwd folds it)"""
    N, H2, W2, Cout = dz.shape
    _lib.check(_lib.load().fp_conv_up2_phase_dgrad_bf3(_f32(dz), _f32(wpacked_bf3), _f32(ext), N, H2 // 2, W2 // 2, Cout, ext.shape[3],
                                                       stream()), "fp_conv_up2_phase_dgrad_bf3")
    return ext


def conv_up2_phase_fwd(low, wphase, bias, y, act=0, addend=None):
    N, h, w, C0 = low.shape
    _lib.check(_lib.load().fp_conv_up2_phase_fwd(_f32(low), _f32(wphase), _f32(bias), _f32(addend), _f32(y), N, h, w, C0, y.shape[3],
                                                 int(act), stream()), "fp_conv_up2_phase_fwd")
    return y


def pack_up2_weight_dgrad(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_up2_weight_dgrad(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()), "fp_pack_up2_weight_dgrad")
    return wp


def pack_conv_weight_dgrad_slice(w, wp, c_begin, c_count):
    Cout, Cin = w.shape[:2]
    _lib.check(_lib.load().fp_pack_conv_weight_dgrad_slice(_f32(w), _f32(wp), Cout, Cin, c_begin, c_count, stream()),
               "fp_pack_conv_weight_dgrad_slice")
    return wp


def up2_fold_bwd(ext, dlow, addend=None, ylow=None, amax_out=None):
    N, h, w, Cn = dlow.shape
    _lib.check(_lib.load().fp_up2_fold_bwd(_f32(ext), N, h, w, Cn, _f32(addend), _f32(ylow), _f32(dlow), _aux(amax_out), stream()), "fp_up2_fold_bwd")
    return dlow


def build_pack_table(jobs, device):
    """jobs: list of (kind, w, wp, c_begin, c_count) over torch tensors that never move.  Returns the device-resident table
    (jobs, blk2job, nblocks) for pack_weights_batched."""
    lib = _lib.load()
    if not jobs:
        return None, None, 0
    arr = (_lib.PackJob * len(jobs))()
    blk2job = []
    for i, job in enumerate(jobs):
        kind, w, wp, c_begin, c_count = job[:5]
        Cout, Cin, KH, KW = w.shape
        nb = lib.fp_pack_job_blocks(kind, Cout, KH, KW, c_count)
        j = arr[i]
        j.w, j.wp = _f32(w), _f32(wp)
        j.Cout, j.Cin, j.KH, j.KW, j.kind, j.c_begin, j.c_count = Cout, Cin, KH, KW, kind, c_begin, c_count
        j.block_begin, j.block_count = len(blk2job), nb
        j.amax = job[5].data_ptr() if len(job) > 5 else None        # fp16-pair kinds: the weight tensor's amax slot
        blk2job += [i] * nb
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    b2j = torch.tensor(blk2job, dtype=torch.int32, device=device)
    return raw, b2j, len(blk2job)


def pack_weights_amax(table):
    """max |w| of every fp16-pair job's weight tensor into its slot (zeroed by the caller); before pack_weights_batched"""
    raw, b2j, nblocks = table
    if nblocks == 0:
        return
    _lib.check(_lib.load().fp_pack_weights_amax(raw.data_ptr(), b2j.data_ptr(), nblocks, stream()), "fp_pack_weights_amax")


def pack_weights_batched(table, max_wgs=0):
    """max_wgs > 0: a persistent launch of at most that many workgroups (a repack on a side stream beside a latency-bound chain)"""
    raw, b2j, nblocks = table
    if nblocks == 0:
        return
    _lib.check(_lib.load().fp_pack_weights_batched_capped(raw.data_ptr(), b2j.data_ptr(), nblocks, int(max_wgs), stream()), "fp_pack_weights_batched")


def colsum(x2d, out, accumulate=False):
    lib = _lib.load()
    M, Cn = x2d.shape
    ws = workspace(lib.fp_colsum_workspace(M, Cn), x2d.device)
    _lib.check(lib.fp_colsum(_f32(x2d), M, Cn, _f32(out), int(bool(accumulate)), ws.data_ptr(), ws.numel(), stream()), "fp_colsum")
    return out


def up2cat_bwd(dxv, N, h, w, C0, C1, dlow, addend=None, ylow=None, dskip=None, accumulate_skip=False):
    _lib.check(_lib.load().fp_up2cat_bwd(_f32(dxv), N, h, w, C0, C1, _f32(addend), _f32(ylow), _f32(dlow), _f32(dskip),
                                         int(bool(accumulate_skip)), stream()), "fp_up2cat_bwd")
    return dlow


def head_fwd(x, w, b, low, sigmoid):
    N, h, wd, Cin = x.shape
    _lib.check(_lib.load().fp_head_fwd(_f32(x), _f32(w), _f32(b), _f32(low), N, h, wd, Cin, int(bool(sigmoid)), stream()), "fp_head_fwd")
    return low


def head_upsample(low, out_nchw, scale, c0):
    N, h, w, _ = low.shape
    _lib.check(_lib.load().fp_head_upsample(_f32(low), _f32(out_nchw), N, h, w, scale, out_nchw.shape[1], c0, stream()), "fp_head_upsample")
    return out_nchw


def head_upsample_bwd(dout_nchw, low, dzlow, scale, c0, sigmoid):
    N, h, w, _ = dzlow.shape
    _lib.check(_lib.load().fp_head_upsample_bwd(_f32(dout_nchw), _f32(low), _f32(dzlow), N, h, w, scale, dout_nchw.shape[1], c0,
                                                int(bool(sigmoid)), stream()), "fp_head_upsample_bwd")
    return dzlow


def head_dgrad(dzlow, w, dx, elu_src=None, amax_out=None):
    N, h, wd, Cin = dx.shape
    _lib.check(_lib.load().fp_head_dgrad(_f32(dzlow), _f32(w), _f32(elu_src), _f32(dx), N, h, wd, Cin, _aux(amax_out), stream()), "fp_head_dgrad")
    return dx


def head_wgrad(x, dzlow, dw, db, accumulate=False):
    lib = _lib.load()
    N, h, wd, Cin = x.shape
    ws = workspace(lib.fp_head_wgrad_workspace(N, h, wd, Cin), x.device)
    _lib.check(lib.fp_head_wgrad(_f32(x), _f32(dzlow), _f32(dw), _f32(db), N, h, wd, Cin, int(bool(accumulate)), ws.data_ptr(),
                                 ws.numel(), stream()), "fp_head_wgrad")


def bn_train_stats(z2d, gamma, beta, running_mean, running_var, nbt, save_mean, save_invstd, scale, shift, eps=1e-5, momentum=0.1):
    lib = _lib.load()
    M, Cn = z2d.shape
    ws = workspace(lib.fp_bn_workspace(M, Cn), z2d.device)
    if nbt is not None and nbt.dtype != torch.int64:
        raise RuntimeError("num_batches_tracked must be int64")
    _lib.check(lib.fp_bn_train_stats(_f32(z2d), M, Cn, _f32(gamma), _f32(beta), eps, momentum, _f32(running_mean), _f32(running_var),
                                     _chk(nbt), _f32(save_mean), _f32(save_invstd), _f32(scale), _f32(shift), ws.data_ptr(),
                                     ws.numel(), stream()), "fp_bn_train_stats")


# statistics out of the producing tile convolution's epilogue (csrc/conv3x3_tile_bf3.hip, fp_aux.bn_part): FP_BN_EPI=0 switches it off
_BN_EPI = bool(int(os.environ.get("FP_BN_EPI", "1")))


def bn_stats_out(part):
    """forward statistics out of the next convolution's epilogue: conv(..., bn_out=bn_stats_out(part)), then `.nblk`"""
    return BnOut(part)


def bn_train_stats_partials(part, nblk, Cn, gamma, beta, running_mean, running_var, nbt, save_mean, save_invstd, scale, shift, eps=1e-5,
                            momentum=0.1):
    if nbt is not None and nbt.dtype != torch.int64:
        raise RuntimeError("num_batches_tracked must be int64")
    _lib.check(_lib.load().fp_bn_train_stats_partials(_f32(part), int(nblk), int(Cn), _f32(gamma), _f32(beta), eps, momentum,
                                                      _f32(running_mean), _f32(running_var), _chk(nbt), _f32(save_mean), _f32(save_invstd),
                                                      _f32(scale), _f32(shift), stream()), "fp_bn_train_stats_partials")


# the BatchNorm-backward reduction out of the producing data gradient's epilogue (csrc/conv3x3_tile_bf3.hip, fp_aux.bnb_*): FP_BN_BWD_EPI=0
# keeps fp_bn_bwd's own reduction pass
_BN_BWD_EPI = bool(int(os.environ.get("FP_BN_BWD_EPI", "1")))


def bn_bwd_out(part, z2d, save_mean, save_invstd):
    """backward sums (sum g, sum g * xhat) out of a tile data gradient's epilogue: conv(..., bn_out=bn_bwd_out(...)), then `.nblk`"""
    return BnOut(part, z2d, save_mean, save_invstd)


def bn_bwd_partials(g2d, z2d, save_mean, save_invstd, gamma, dz2d, dgamma, dbeta, part, nblk, accumulate=False, amax_out=None):
    """fp_bn_bwd without its reduction pass: g2d is already masked, `part` holds (sum g, sum g * xhat) per pixel tile and channel"""
    lib = _lib.load()
    M, Cn = z2d.shape
    coef = workspace(lib.fp_bn_workspace(M, Cn), z2d.device)
    _lib.check(lib.fp_bn_bwd_partials(_f32(g2d), _f32(z2d), _f32(save_mean), _f32(save_invstd), _f32(gamma), _f32(dz2d), _f32(dgamma),
                                      _f32(dbeta), int(bool(accumulate)), M, Cn, _f32(part), int(nblk), coef.data_ptr(), _aux(amax_out), stream()),
               "fp_bn_bwd_partials")
    return dz2d


def bn_eval_coeffs(gamma, beta, rm, rv, scale, shift, eps=1e-5):
    _lib.check(_lib.load().fp_bn_eval_coeffs(_f32(gamma), _f32(beta), _f32(rm), _f32(rv), eps, gamma.numel(), _f32(scale), _f32(shift),
                                             stream()), "fp_bn_eval_coeffs")


def bn_eval_coeffs_saved(gamma, beta, rm, rv, scale, shift, save_mean, save_invstd, eps=1e-5):
    """bn_eval_coeffs for a forward that a backward pass follows (frozen statistics): also save_mean = rm, save_invstd = 1 / sqrt(rv + eps)"""
    _lib.check(_lib.load().fp_bn_eval_coeffs_saved(_f32(gamma), _f32(beta), _f32(rm), _f32(rv), eps, gamma.numel(), _f32(scale), _f32(shift),
                                                   _f32(save_mean), _f32(save_invstd), stream()), "fp_bn_eval_coeffs_saved")


def bn_bwd_frozen(dy2d, relu_out, z2d, mean, invstd, gamma, dz2d, dgamma, dbeta, g_out=None, accumulate=False, amax_out=None):
    """backward of a BatchNorm that normalised with (mean, invstd) = its running statistics: dz = g * gamma * invstd in one pass; the sums
    dgamma / dbeta (each optional) from the same pass.  With neither, z2d / mean may be None and are not read."""
    lib = _lib.load()
    M, Cn = dy2d.shape
    ws_ptr, ws_n = 0, 0
    if dgamma is not None or dbeta is not None:
        ws = workspace(lib.fp_bn_workspace(M, Cn), dy2d.device)
        ws_ptr, ws_n = ws.data_ptr(), ws.numel()
    _lib.check(lib.fp_bn_bwd_frozen(_f32(dy2d), _f32(relu_out), _f32(z2d), _f32(mean), _f32(invstd), _f32(gamma), _f32(dz2d), _f32(dgamma),
                                    _f32(dbeta), _f32(g_out), int(bool(accumulate)), M, Cn, ws_ptr, ws_n, _u32(amax_out, "amax_out"), stream()),
               "fp_bn_bwd_frozen")
    return dz2d


def bn_bwd_frozen_partials(g2d, invstd, gamma, dz2d, dgamma, dbeta, part, nblk, accumulate=False, amax_out=None):
    """bn_bwd_frozen on a masked g whose producer wrote the partial sums (sum g, sum g * xhat) per pixel tile and channel"""
    M, Cn = g2d.shape
    _lib.check(_lib.load().fp_bn_bwd_frozen_partials(_f32(g2d), _f32(invstd), _f32(gamma), _f32(dz2d), _f32(dgamma), _f32(dbeta),
                                                     int(bool(accumulate)), M, Cn, _f32(part), int(nblk), _u32(amax_out, "amax_out"), stream()),
               "fp_bn_bwd_frozen_partials")
    return dz2d


def scale_rows(w, scale, out):
    rows = w.shape[0]
    _lib.check(_lib.load().fp_scale_rows(_f32(w), _f32(scale), _f32(out), rows, w.numel() // rows, stream()), "fp_scale_rows")
    return out


def bn_apply(z2d, scale, shift, y2d, residual=None, relu=True, amax_out=None):
    M, Cn = z2d.shape
    _lib.check(_lib.load().fp_bn_apply(_f32(z2d), _f32(scale), _f32(shift), _f32(residual), _f32(y2d), M, Cn, int(bool(relu)), _aux(amax_out), stream()),
               "fp_bn_apply")
    return y2d


def bn_bwd(dy2d, relu_out, z2d, save_mean, save_invstd, gamma, dz2d, dgamma, dbeta, g_out=None, accumulate=False, amax_out=None):
    """amax_out: slot receiving max |dz| (the apply stage publishes it)"""
    lib = _lib.load()
    M, Cn = z2d.shape
    ws = workspace(lib.fp_bn_workspace(M, Cn), z2d.device)
    _lib.check(lib.fp_bn_bwd(_f32(dy2d), _f32(relu_out), _f32(z2d), _f32(save_mean), _f32(save_invstd), _f32(gamma), _f32(dz2d),
                             _f32(g_out), _f32(dgamma), _f32(dbeta), int(bool(accumulate)), M, Cn, ws.data_ptr(), ws.numel(), _aux(amax_out), stream()),
               "fp_bn_bwd")
    return dz2d


def maxpool_fwd(x, y, argmax, amax_out=None):
    N, H, W, Cn = x.shape
    _lib.check(_lib.load().fp_maxpool_fwd(_f32(x), _f32(y), _chk(argmax), N, H, W, Cn, _aux(amax_out), stream()), "fp_maxpool_fwd")
    return y


def maxpool_bwd(dy, argmax, dx, accumulate=False):
    N, H, W, Cn = dx.shape
    _lib.check(_lib.load().fp_maxpool_bwd(_f32(dy), _chk(argmax), _f32(dx), N, H, W, Cn, int(bool(accumulate)), stream()), "fp_maxpool_bwd")
    return dx


def loss_fwd_bwd(preds, targets, losses_out, dpreds=None, depth_range=(0.1, 100.0), prior=0.25):
    """preds: 4 tensors [B,4,H,W] in order '1/8','1/4','1/2','1/1'; targets: dict with the reference batch keys."""
    lib = _lib.load()
    B, _, H, W = preds[0].shape
    ws = workspace(lib.fp_loss_workspace(B, H, W), preds[0].device)
    P = (C.c_void_p * 4)(*[_f32(p, "pred") for p in preds])
    D = (C.c_void_p * 4)(*[_f32(p, "dpred") for p in dpreds]) if dpreds is not None else None
    _lib.check(lib.fp_loss_fwd_bwd(P, _f32(targets["visible_ground"]), _f32(targets["all_ground"]), _f32(targets["depth"]),
                                   _f32(targets["ground_depth"]), _f32(targets["moving_object_mask"]), _f32(targets["depth_mask"]),
                                   float(depth_range[0]), float(depth_range[1]), float(prior), D, _f32(losses_out), B, H, W,
                                   ws.data_ptr(), ws.numel(), stream()), "fp_loss_fwd_bwd")
    return losses_out


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0):
    _lib.check(_lib.load().fp_adam_step(_f32(param), _f32(grad), _f32(exp_avg), _f32(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
                                        int(step), grad_scale, stream()), "fp_adam_step")


def adam_hyper(lr, beta1, beta2, eps, step, grad_scale=1.0):
    """the seven float scalars of one Adam step (host tensor), derived exactly like fp_adam_step does"""
    h = torch.empty(7, dtype=torch.float32)
    _lib.check(_lib.load().fp_adam_hyper(lr, beta1, beta2, eps, int(step), grad_scale, h.data_ptr()), "fp_adam_hyper")
    return h


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, hyper_dev):
    _lib.check(_lib.load().fp_adam_step_dev(_f32(param), _f32(grad), _f32(exp_avg), _f32(exp_avg_sq), param.numel(), _f32(hyper_dev),
                                            stream()), "fp_adam_step_dev")


def pack_pred_fp16(pred, out=None):
    """[B,4,H,W] fp32 network output -> float16 with sigmoid on the mask channels (the test-set inference file format)"""
    B, Cn, H, W = pred.shape
    if Cn != 4:
        raise RuntimeError("pack_pred_fp16 expects the 4-channel network output")
    if out is None:
        out = torch.empty((B, 4, H, W), dtype=torch.float16, device=pred.device)
    _lib.check(_lib.load().fp_pack_pred_fp16(_f32(pred), _chk(out), B, H, W, stream()), "fp_pack_pred_fp16")
    return out


def eval_mask_counts(pred, gt, region=None, invert=False):
    """pred [B,H,W] float16/float32 (may be a channel slice of [B,4,H,W]), gt [B,H,W] float32, region [B,H,W] uint8 or None
    -> int64 [B,4] = n_true, tp, fp, fn (evaluate_model.py:72-99 thresholds)"""
    B = pred.shape[0]
    pixels = pred.shape[1] * pred.shape[2]
    if pred.dtype not in (torch.float16, torch.float32) or pred.stride(2) != 1 or pred.stride(1) != pred.shape[2]:
        raise RuntimeError("eval_mask_counts: pred must be float16/float32 with contiguous images")
    if region is not None and (region.dtype != torch.uint8 or tuple(region.shape) != tuple(gt.shape)):
        raise RuntimeError("eval_mask_counts: region must be uint8 with the ground truth's shape")
    if not pred.is_cuda:
        raise RuntimeError("eval_mask_counts: pred must be a CUDA tensor (no CPU path in the product)")
    counts = torch.empty((B, 4), dtype=torch.int64, device=pred.device)
    _lib.check(_lib.load().fp_eval_mask_counts(pred.data_ptr(), int(pred.dtype == torch.float16), _f32(gt), _chk(region) if region is not None else None,
                                               int(bool(invert)), B, pixels, pred.stride(0), _chk(counts), stream()), "fp_eval_mask_counts")
    return counts


def eval_depth_sums(disp, gt, min_depth=0.1, max_depth=100.0, clip=(0.5, 20.0)):
    """disp [B,H,W] float16/float32 sigmoid output, gt [B,H,W] float32 -> float64 [B,5] = n, n(a1), sum sq, sum abs_rel, sum sq_rel"""
    B = disp.shape[0]
    pixels = disp.shape[1] * disp.shape[2]
    if disp.dtype not in (torch.float16, torch.float32) or disp.stride(2) != 1 or disp.stride(1) != disp.shape[2]:
        raise RuntimeError("eval_depth_sums: disp must be float16/float32 with contiguous images")
    if not disp.is_cuda:
        raise RuntimeError("eval_depth_sums: disp must be a CUDA tensor (no CPU path in the product)")
    sums = torch.empty((B, 5), dtype=torch.float64, device=disp.device)
    _lib.check(_lib.load().fp_eval_depth_sums(disp.data_ptr(), int(disp.dtype == torch.float16), _f32(gt), B, pixels, disp.stride(0), float(min_depth),
                                              float(max_depth), float(clip[0]), float(clip[1]), _chk(sums), stream()), "fp_eval_depth_sums")
    return sums


def nchw_to_nhwc(x, y=None):
    N, Cn, H, W = x.shape
    if y is None:
        y = torch.empty((N, H, W, Cn), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().fp_nchw_to_nhwc(_f32(x), _f32(y), N, Cn, H, W, stream()), "fp_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x, y=None):
    N, H, W, Cn = x.shape
    if y is None:
        y = torch.empty((N, Cn, H, W), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().fp_nhwc_to_nchw(_f32(x), _f32(y), N, Cn, H, W, stream()), "fp_nhwc_to_nchw")
    return y


def fill(x, value):
    _lib.check(_lib.load().fp_fill(_f32(x), x.numel(), float(value), stream()), "fp_fill")
    return x


# ---- pyramid pooling (segmentation network, footprints/preprocessing/segmentation/network.py:174-207) -------------------------
def adaptive_avgpool_fwd(x, y):
    N, H, W, Cn = x.shape
    P = y.shape[1]
    _lib.check(_lib.load().fp_adaptive_avgpool_fwd(_f32(x), _f32(y), N, H, W, Cn, P, stream()), "fp_adaptive_avgpool_fwd")
    return y


def adaptive_avgpool_bwd(dy, dx, accumulate=False):
    N, H, W, Cn = dx.shape
    P = dy.shape[1]
    _lib.check(_lib.load().fp_adaptive_avgpool_bwd(_f32(dy), _f32(dx), N, H, W, Cn, P, int(bool(accumulate)), stream()), "fp_adaptive_avgpool_bwd")
    return dx


def bilinear_ac_fwd(src, dst, c_off):
    """src [N,P,P,C] -> dst[N,H,W,dstC][..., c_off:c_off+C] (bilinear, align_corners=True)"""
    N, P, _, Cn = src.shape
    _, H, W, dstC = dst.shape
    _lib.check(_lib.load().fp_bilinear_ac_fwd(_f32(src), _f32(dst), N, P, Cn, H, W, dstC, c_off, stream()), "fp_bilinear_ac_fwd")
    return dst


def bilinear_ac_bwd(ddst, dsrc, c_off):
    N, P, _, Cn = dsrc.shape
    _, H, W, dstC = ddst.shape
    _lib.check(_lib.load().fp_bilinear_ac_bwd(_f32(ddst), _f32(dsrc), N, P, Cn, H, W, dstC, c_off, stream()), "fp_bilinear_ac_bwd")
    return dsrc


def copy_channels(src, dst, C_, src_off=0, dst_off=0, accumulate=False):
    """dst[..., dst_off:dst_off+C] (+)= src[..., src_off:src_off+C] for NHWC tensors with equal pixel counts"""
    srcC, dstC = src.shape[-1], dst.shape[-1]
    M = src.numel() // srcC
    if dst.numel() // dstC != M:
        raise RuntimeError("copy_channels: pixel counts differ")
    _lib.check(_lib.load().fp_copy_channels(_f32(src), _f32(dst), M, C_, srcC, src_off, dstC, dst_off, int(bool(accumulate)), stream()),
               "fp_copy_channels")
    return dst


def seg_loss_fwd_bwd(preds, ground_mask, loss_mask, losses_out, dpreds=None):
    """segmentation trainer's loss (+ gradient): preds = four logit maps [B,1,h,w] (any batch stride: channel slices of wider buffers
    are fine as long as a map's rows are dense), masks [B,H,W]; losses_out: 5 B + 1 floats (per-scale / per-image means, their average,
    batch mean); dpreds: four tensors addressed like preds, or None"""
    lib = _lib.load()
    B, H, W = ground_mask.shape
    for t in list(preds) + (list(dpreds) if dpreds is not None else []):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 1 and t.stride(3) == 1 and t.stride(2) == t.shape[3]):
            raise RuntimeError("footprints_amd.ops.seg_loss_fwd_bwd: maps must be float32 CUDA [B,1,h,w] with dense rows")
    ws = workspace(lib.fp_seg_loss_workspace(B, H, W), ground_mask.device)
    P = (C.c_void_p * 4)(*[p.data_ptr() for p in preds])
    D = (C.c_void_p * 4)(*[p.data_ptr() for p in dpreds]) if dpreds is not None else None
    hs = (C.c_int32 * 4)(*[p.shape[2] for p in preds])
    wss = (C.c_int32 * 4)(*[p.shape[3] for p in preds])
    bs = (C.c_int64 * 4)(*[p.stride(0) if B > 1 else p.shape[2] * p.shape[3] for p in preds])      # a batch of one has no batch stride
    if dpreds is not None and B > 1 and any(d.stride(0) != p.stride(0) for d, p in zip(dpreds, preds)):
        raise RuntimeError("footprints_amd.ops.seg_loss_fwd_bwd: gradient maps must be addressed like the predictions")
    _lib.check(lib.fp_seg_loss_fwd_bwd(P, D, hs, wss, bs, _f32(ground_mask), _f32(loss_mask), B, H, W, _f32(losses_out), ws.data_ptr(), ws.numel(),
                                       stream()), "fp_seg_loss_fwd_bwd")
    return losses_out


# ---- training-label generation (csrc/gt_gen.hip; semantics in include/footprints_hip.h) ----------------------------------------------
def _typed(t, dtype, name):
    if t is not None and t.dtype != dtype:
        raise RuntimeError("footprints_amd.ops: %s must be %s" % (name, dtype))
    return _chk(t, name)


def gt_workspace_bytes(B, H, W):
    """bytes of key plane for B frames of H x W (host-only query; raises on B > 512 or H * W * 64 >= 2^32 - 1)"""
    n = _lib.load().fp_gt_workspace(B, H, W)
    if n < 0:
        _lib.check(-1, "fp_gt_workspace")
    return n


def gt_keys(B, H, W, device):
    """a key plane of its own (uint64 as int64 [B, H*W]): the splats fill it, gt_aggregate / gt_depth_mask read it"""
    return torch.empty(gt_workspace_bytes(B, H, W) // 8, dtype=torch.int64, device=device).view(B, H * W)


def _gt_mats(B, **mats):
    out = []
    for name, m in mats.items():
        if tuple(m.shape) != (B, 4, 4):
            raise RuntimeError("footprints_amd.ops: %s must be [%d, 4, 4]" % (name, B))
        out.append(_f32(m, name))
    return out


def gt_project(depths, inv_intrinsics, poses, intrinsics):
    """depths [B,H,W] -> cam_pix [B,4,H*W] = u, v, z, c3 (the staged warp)"""
    B, H, W = depths.shape
    iK, T, K = _gt_mats(B, inv_intrinsics=inv_intrinsics, poses=poses, intrinsics=intrinsics)
    d = _f32(depths, "depths")
    cam_pix = torch.empty((B, 4, H * W), dtype=torch.float32, device=depths.device)
    _lib.check(_lib.load().fp_gt_project(d, iK, T, K, B, H, W, _chk(cam_pix), stream()), "fp_gt_project")
    return cam_pix


def gt_project_to_world(depths, inv_intrinsics):
    """depths [B,H,W] -> world points [B,4,H*W] = (invK[:3,:3] . (x, y, 1)) * d and the homogeneous (d > 0)"""
    B, H, W = depths.shape
    (iK,) = _gt_mats(B, inv_intrinsics=inv_intrinsics)
    d = _f32(depths, "depths")
    world = torch.empty((B, 4, H * W), dtype=torch.float32, device=depths.device)
    _lib.check(_lib.load().fp_gt_project_to_world(d, iK, B, H, W, _chk(world), stream()), "fp_gt_project_to_world")
    return world


def gt_project_to_camera(world, poses, intrinsics):
    """world points [B,4,N] -> cam_pix [B,4,N] = K . (T . world) with u, v divided by (z + 1e-7)"""
    B, four, N = world.shape
    if four != 4:
        raise RuntimeError("footprints_amd.ops.gt_project_to_camera: world points must be [B, 4, N]")
    T, K = _gt_mats(B, poses=poses, intrinsics=intrinsics)
    w = _f32(world, "world points")
    cam_pix = torch.empty((B, 4, N), dtype=torch.float32, device=world.device)
    _lib.check(_lib.load().fp_gt_project_to_camera(w, T, K, B, N, _chk(cam_pix), stream()), "fp_gt_project_to_camera")
    return cam_pix


def gt_splat(cam_pix, H, W, keys=None):
    """cam_pix [B,4,H*W] -> keys [B,H*W] (highest source index wins a pixel)"""
    B = cam_pix.shape[0]
    if tuple(cam_pix.shape) != (B, 4, H * W):
        raise RuntimeError("footprints_amd.ops.gt_splat: cam_pix must be [B, 4, H*W]")
    c = _f32(cam_pix, "cam_pix")
    keys = gt_keys(B, H, W, cam_pix.device) if keys is None else keys
    _lib.check(_lib.load().fp_gt_splat(c, B, H, W, _typed(keys, torch.int64, "keys"), keys.numel() * 8, stream()), "fp_gt_splat")
    return keys


def gt_warp_splat(depths, inv_intrinsics, poses, intrinsics, keys=None):
    """the production path: warp and splat in one kernel, depths [B,H,W] -> keys [B,H*W]"""
    B, H, W = depths.shape
    iK, T, K = _gt_mats(B, inv_intrinsics=inv_intrinsics, poses=poses, intrinsics=intrinsics)
    d = _f32(depths, "depths")
    keys = gt_keys(B, H, W, depths.device) if keys is None else keys
    _lib.check(_lib.load().fp_gt_warp_splat(d, iK, T, K, B, H, W, _typed(keys, torch.int64, "keys"), keys.numel() * 8, stream()),
               "fp_gt_warp_splat")
    return keys


def gt_aggregate(keys, H, W, robust, want_projections=False):
    """keys [B,H*W] -> median [H,W] (and the per-frame projections [B,H,W] when asked)"""
    B = keys.shape[0]
    if keys.numel() != B * H * W:
        raise RuntimeError("footprints_amd.ops.gt_aggregate: keys must be [B, H*W]")
    k = _typed(keys, torch.int64, "keys")
    median = torch.empty((H, W), dtype=torch.float32, device=keys.device)
    proj = torch.empty((B, H, W), dtype=torch.float32, device=keys.device) if want_projections else None
    _lib.check(_lib.load().fp_gt_aggregate(k, B, H, W, int(bool(robust)), _chk(median), _chk(proj) if proj is not None else None, stream()),
               "fp_gt_aggregate")
    return (median, proj) if want_projections else median


def gt_moving_mask(disparity, flow, inv_intrinsics, pose, intrinsics, fx_baseline):
    """disparity [H,W], flow [2,H,W], matrices [1,4,4] -> bool [H,W]"""
    H, W = disparity.shape[-2:]
    if disparity.numel() != H * W or tuple(flow.shape) != (2, H, W):
        raise RuntimeError("footprints_amd.ops.gt_moving_mask: disparity must be [H, W] and flow [2, H, W]")
    iK, T, K = _gt_mats(1, inv_intrinsics=inv_intrinsics, pose=pose, intrinsics=intrinsics)
    d, f = _f32(disparity, "disparity"), _f32(flow, "flow")
    mask = torch.empty((H, W), dtype=torch.uint8, device=disparity.device)
    _lib.check(_lib.load().fp_gt_moving_mask(d, f, iK, T, K, float(fx_baseline), H, W, _chk(mask), stream()), "fp_gt_moving_mask")
    return mask.view(torch.bool)


def gt_ground_count(ground_seg, threshold):
    """number of pixels with ground_seg > threshold (int32 device scalar)"""
    H, W = ground_seg.shape
    g = _f32(ground_seg, "ground_seg")
    count = torch.empty(1, dtype=torch.int32, device=ground_seg.device)
    _lib.check(_lib.load().fp_gt_ground_count(g, float(threshold), H, W, _chk(count), stream()), "fp_gt_ground_count")
    return count


def gt_plane_score(world, ground_seg, threshold, samples, want_inlier_mask=False):
    """world [4,H*W] (one frame of gt_project_to_world), ground_seg [H,W], samples int32 [C,3] (indices into the ground pixels in raster order) -> dict of sample_pix [C,3],
    planes float64 [C,4], counts int32 [C], best_plane float64 [4], best int32 [2] = (index, count), inlier_mask bool [H,W] or None"""
    H, W = ground_seg.shape
    if world.numel() != 4 * H * W or samples.dim() != 2 or samples.shape[1] != 3:
        raise RuntimeError("footprints_amd.ops.gt_plane_score: world must be [4, H*W] and samples [C, 3]")
    d, g, s = _f32(world, "world points"), _f32(ground_seg, "ground_seg"), _typed(samples, torch.int32, "samples")
    C_, dev = samples.shape[0], world.device
    out = {"sample_pix": torch.empty((C_, 3), dtype=torch.int32, device=dev), "planes": torch.empty((C_, 4), dtype=torch.float64, device=dev),
           "counts": torch.empty(C_, dtype=torch.int32, device=dev), "best_plane": torch.empty(4, dtype=torch.float64, device=dev),
           "best": torch.empty(2, dtype=torch.int32, device=dev),
           "inlier_mask": torch.empty((H, W), dtype=torch.uint8, device=dev) if want_inlier_mask else None}
    _lib.check(_lib.load().fp_gt_plane_score(d, g, float(threshold), s, C_, H, W, _chk(out["sample_pix"]), _chk(out["planes"]),
                                             _chk(out["counts"]), _chk(out["best_plane"]), _chk(out["best"]),
                                             _chk(out["inlier_mask"]) if want_inlier_mask else None, stream()), "fp_gt_plane_score")
    if want_inlier_mask:
        out["inlier_mask"] = out["inlier_mask"].view(torch.bool)
    return out


def gt_flatten_splat(world, ground_seg, threshold, intrinsics, plane, keys=None, want_cam_pix=False):
    """non-ground points of `world` [4,H*W] flattened onto `plane` (float64 [4] on the device), 8 x 8 offset copies projected and splatted -> keys [1,H*W]
    (and the copies' coordinates [4, 64*H*W] when asked: tests only)"""
    H, W = ground_seg.shape
    if world.numel() != 4 * H * W:
        raise RuntimeError("footprints_amd.ops.gt_flatten_splat: world must be [4, H*W]")
    (K,) = _gt_mats(1, intrinsics=intrinsics)
    d, g, pl = _f32(world, "world points"), _f32(ground_seg, "ground_seg"), _typed(plane, torch.float64, "plane")
    if plane.numel() != 4:
        raise RuntimeError("footprints_amd.ops.gt_flatten_splat: plane must hold 4 float64")
    keys = gt_keys(1, H, W, world.device) if keys is None else keys
    cam_pix = torch.empty((4, 64 * H * W), dtype=torch.float32, device=world.device) if want_cam_pix else None
    _lib.check(_lib.load().fp_gt_flatten_splat(d, g, float(threshold), K, pl, H, W, _typed(keys, torch.int64, "keys"), keys.numel() * 8,
                                               _chk(cam_pix) if want_cam_pix else None, stream()), "fp_gt_flatten_splat")
    return (keys, cam_pix) if want_cam_pix else keys


def gt_depth_mask(keys, depth, ground_seg, want_projection=False):
    """keys [1,H*W] of gt_flatten_splat -> bool [H,W] mask of untraversable pixels (and the splatted projection when asked)"""
    H, W = ground_seg.shape
    if depth.numel() != H * W or keys.numel() < H * W:
        raise RuntimeError("footprints_amd.ops.gt_depth_mask: depth must be [H, W] and keys hold H*W entries")
    k, d, g = _typed(keys, torch.int64, "keys"), _f32(depth, "depth"), _f32(ground_seg, "ground_seg")
    mask = torch.empty((H, W), dtype=torch.uint8, device=depth.device)
    proj = torch.empty((H, W), dtype=torch.float32, device=depth.device) if want_projection else None
    _lib.check(_lib.load().fp_gt_depth_mask(k, d, g, H, W, _chk(mask), _chk(proj) if want_projection else None, stream()), "fp_gt_depth_mask")
    return (mask.view(torch.bool), proj) if want_projection else mask.view(torch.bool)


# ---- the paper's comparison baselines (csrc/baselines.hip; semantics in include/footprints_hip.h) --------------------------------------
_BASELINE_DTYPES = {torch.uint8: 0, torch.bool: 0, torch.float16: 1, torch.float32: 2}


def _baseline_mask(t, threshold, name, shape=None):
    """-> (pointer, dtype code, threshold) of a [B,H,W] mask: uint8 / bool (non-zero is set) or float16 / float32 with a threshold"""
    if t.dtype not in _BASELINE_DTYPES:
        raise RuntimeError("footprints_amd.ops: %s must be uint8, bool, float16 or float32" % name)
    if t.dim() != 3 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError("footprints_amd.ops: %s must be [B, H, W]%s" % (name, "" if shape is None else " = %s" % (tuple(shape),)))
    code = _BASELINE_DTYPES[t.dtype]
    if code and threshold is None:
        raise RuntimeError("footprints_amd.ops: a floating-point %s needs a threshold" % name)
    return _chk(t, name), code, float(threshold) if code else 0.0


def convex_hull_mask(x, threshold=None, remove=None, keep=None):
    """x [B,H,W] uint8 / bool, or float16 / float32 with `threshold` (x > threshold in x's dtype) -> uint8 [B,H,W], each frame
    skimage.morphology.convex_hull_image of its mask (zeros for an empty one), exact.  BoundingBox's epilogue in the same pass:
    pixels with `remove` < 0.5 are cleared, then pixels set in `keep` (a mask like x, same threshold) are set."""
    xp, xd, xt = _baseline_mask(x, threshold, "mask")
    B, H, W = x.shape
    rp = rd = kp = kd = 0
    kt = 0.0
    if remove is not None:
        rp, rd, _ = _baseline_mask(remove, 0.5, "remove", x.shape)
    if keep is not None:
        kp, kd, kt = _baseline_mask(keep, threshold, "keep", x.shape)
    spans = torch.empty((B, H, 2), dtype=torch.int32, device=x.device)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().fp_baseline_hull(xp, xd, xt, rp or None, rd, kp or None, kd, kt, B, H, W, _chk(spans), _chk(out), stream()),
               "fp_baseline_hull")
    return out


def baseline_mask_counts(x, threshold=None):
    """set pixels of every frame of the mask x [B,H,W] -> int32 [B] on the device"""
    xp, xd, xt = _baseline_mask(x, threshold, "mask")
    B, H, W = x.shape
    counts = torch.empty(B, dtype=torch.int32, device=x.device)
    _lib.check(_lib.load().fp_baseline_mask_counts(xp, xd, xt, B, H, W, _chk(counts), stream()), "fp_baseline_mask_counts")
    return counts


def _baseline_frames(depth, inv_K):
    B, H, W = depth.shape
    if tuple(inv_K.shape) != (B, 3, 3):
        raise RuntimeError("footprints_amd.ops: inv_K must be float64 [%d, 3, 3]" % B)
    return _f32(depth, "depth"), _typed(inv_K, torch.float64, "inv_K"), B, H, W


def baseline_plane_fit(depth, inv_K, mask, samples, threshold=0.5):
    """ransac.run_ransac over a batch: depth float32 [B,H,W], inv_K float64 [B,3,3], mask [B,H,W] (see convex_hull_mask), samples int32
    [B,C,3] = ranks into each frame's masked pixels in raster order -> dict of sample_pix [B,C,3], planes float64 [B,C,4] (unit 4-vectors),
    counts int32 [B,C], best int32 [B,2] = (index, count) and best_plane float64 [B,4]"""
    d, iK, B, H, W = _baseline_frames(depth, inv_K)
    mp, md, mt = _baseline_mask(mask, threshold, "mask", depth.shape)
    if samples.dim() != 3 or samples.shape[0] != B or samples.shape[2] != 3:
        raise RuntimeError("footprints_amd.ops.baseline_plane_fit: samples must be int32 [B, C, 3]")
    s = _typed(samples, torch.int32, "samples")
    C_, dev = samples.shape[1], depth.device
    out = {"sample_pix": torch.empty((B, C_, 3), dtype=torch.int32, device=dev), "planes": torch.empty((B, C_, 4), dtype=torch.float64, device=dev),
           "counts": torch.empty((B, C_), dtype=torch.int32, device=dev), "best": torch.empty((B, 2), dtype=torch.int32, device=dev),
           "best_plane": torch.empty((B, 4), dtype=torch.float64, device=dev)}
    _lib.check(_lib.load().fp_baseline_plane_fit(d, iK, mp, md, mt, s, C_, B, H, W, _chk(out["sample_pix"]), _chk(out["planes"]), _chk(out["counts"]),
                                                 _chk(out["best_plane"]), _chk(out["best"]), stream()), "fp_baseline_plane_fit")
    return out


def baseline_plane_depth(depth, inv_K, best_plane, passthrough=None):
    """depth of the plane along every pixel's ray (footprint_baseline.ransac_depth_inpaint): float64 [B,H,W]; frames with a non-zero
    `passthrough` (uint8 / bool [B]) get their input depth"""
    d, iK, B, H, W = _baseline_frames(depth, inv_K)
    if tuple(best_plane.shape) != (B, 4):
        raise RuntimeError("footprints_amd.ops.baseline_plane_depth: best_plane must be float64 [B, 4]")
    pl = _typed(best_plane, torch.float64, "best_plane")
    pt = None
    if passthrough is not None:
        if passthrough.dtype not in (torch.uint8, torch.bool) or tuple(passthrough.shape) != (B,):
            raise RuntimeError("footprints_amd.ops.baseline_plane_depth: passthrough must be uint8 or bool [B]")
        pt = _chk(passthrough, "passthrough")
    out = torch.empty((B, H, W), dtype=torch.float64, device=depth.device)
    _lib.check(_lib.load().fp_baseline_plane_depth(d, iK, pl, pt, B, H, W, _chk(out), stream()), "fp_baseline_plane_depth")
    return out


# ---- reader work on the device: Pillow's 8-bit resize (csrc/resample_u8.hip) and filter_depth_mask (csrc/reader.hip) ------------------
RESIZE_FILTERS = {"lanczos": _lib.RESIZE_LANCZOS, "bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC, "box": _lib.RESIZE_BOX}
_resize_host_tables = {}


def _status_word(ws, off):
    """the int32 a resize call left at byte `off` of its workspace (WAITS for the stream)"""
    return int(ws[off:off + 4].view(torch.int32).item())


def _resize_filter(f):
    f = RESIZE_FILTERS.get(f, f) if isinstance(f, str) else int(f)
    if f not in RESIZE_FILTERS.values():
        raise ValueError("footprints_amd.ops: resize filter must be one of %s (or Pillow's number of one)" % sorted(RESIZE_FILTERS))
    return f


def resize_tables(in_size, out_size, filter="lanczos"):
    """Pillow's coefficient tables of one axis, built by the library on the host in double (no GPU needed) and cached per
    (in, out, filter) -> (bounds int32 [out, 2] = first source index and tap count, kk int32 [out, ksize] in 22-bit fixed point)"""
    import numpy as np
    key = (int(in_size), int(out_size), _resize_filter(filter))
    t = _resize_host_tables.get(key)
    if t is None:
        lib = _lib.load()
        ksize = lib.fp_resize_ksize(*key)
        if ksize < 0:
            raise ValueError("footprints_amd.ops.resize_tables: bad sizes %r" % (key,))
        bounds, kk = np.empty((key[1], 2), np.int32), np.empty((key[1], ksize), np.int32)
        _lib.check(lib.fp_resize_coeffs(key[0], key[1], key[2], bounds.ctypes.data, kk.ctypes.data, ksize), "fp_resize_coeffs")
        bounds.setflags(write=False)
        kk.setflags(write=False)
        t = _resize_host_tables[key] = (bounds, kk)
    return t


class ResizeTableSet:
    """The axis tables one device has seen, in one int32 buffer plus one fp_resize_table record each.  `index` is host work (fill time);
    `device()` uploads when a table was added since the last upload -- once per distinct (in, out, filter) -- on the current stream."""

    def __init__(self, device):
        import threading
        self.device = torch.device(device)
        self.lock = threading.Lock()           # a loader's worker thread asks for indices while the main thread uploads
        self.keys, self.records, self.coeffs, self.length = {}, [], [], 0
        self.uploaded, self.d_tables, self.d_coeffs = 0, None, None

    def index(self, in_size, out_size, filter="lanczos"):
        """index of the (in -> out) table; -1 when the sizes agree (the pass is skipped, as in Pillow)"""
        if in_size == out_size:
            return -1
        key = (int(in_size), int(out_size), _resize_filter(filter))
        with self.lock:
            i = self.keys.get(key)
            if i is None:
                bounds, kk, ksize = self._host_tables(key)
                i = self.keys[key] = len(self.records)
                self.records.append(_lib.ResizeTable(key[0], key[1], ksize, self.length, self.length + bounds.size))
                self.coeffs += [bounds, kk]
                self.length += bounds.size + kk.size
        return i

    def _host_tables(self, key):
        """(bounds, kk, ksize) of one axis as flat arrays of the buffer's element type"""
        bounds, kk = resize_tables(*key)
        return bounds.reshape(-1), kk.reshape(-1), kk.shape[1]

    def device_buffers(self):
        """(table records, count, coefficient buffer) on the device"""
        import numpy as np
        with self.lock:
            n = len(self.records)
            if n != self.uploaded:
                # queued launches may still read the superseded buffers: let go of them as every replaced device buffer is
                release(self.d_tables, "resize_tables")
                release(self.d_coeffs, "resize_coeffs")
                rec = np.frombuffer(b"".join(bytes(r) for r in self.records), dtype=np.uint8).copy()
                self.d_tables = torch.from_numpy(rec).to(self.device)
                self.d_coeffs = torch.from_numpy(np.concatenate(self.coeffs)).to(self.device)
                self.uploaded = n
                bump_alloc_generation()
            return self.d_tables, n, self.d_coeffs


_resize_table_sets = {}


def resize_table_set(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _resize_table_sets.get(device)
    if s is None:
        assert _lib.load().fp_resize_table_bytes() == C.sizeof(_lib.ResizeTable) and _lib.load().fp_resize_sample_bytes() == C.sizeof(_lib.ResizeSample)
        s = _resize_table_sets[device] = ResizeTableSet(device)
    return s


def resize_pack(images, H, W, tables, filter="lanczos", packed=None, records=None):
    """host half of a resize: the images (uint8 [h, w, C] or [h, w], all the same C) one after the other in `packed` (a uint8 numpy
    buffer, allocated when None) and their fp_resize_sample records in `records` (uint8 numpy view, allocated when None)
    -> (packed, records, bytes used, C, max_h, max_w)"""
    import numpy as np
    B = len(images)
    shapes = [(im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2]) for im in images]
    Cn = shapes[0][2]
    if Cn not in (1, 3) or any(s[2] != Cn for s in shapes) or any(im.dtype != np.uint8 for im in images):
        raise ValueError("footprints_amd.ops.resize_pack: images must be uint8 [h, w] or [h, w, C] with one C of 1 or 3")
    total = sum(h * w * c for h, w, c in shapes)
    if packed is None:
        packed = np.empty(total, np.uint8)
    if total > packed.size:
        raise ValueError("footprints_amd.ops.resize_pack: the batch needs %d source bytes, the buffer holds %d" % (total, packed.size))
    rec = (_lib.ResizeSample * B)()
    off = 0
    for b, (im, (h, w, c)) in enumerate(zip(images, shapes)):
        packed[off:off + h * w * c] = im.reshape(-1)
        rec[b] = _lib.ResizeSample(off, h, w, tables.index(w, W, filter), tables.index(h, H, filter))
        off += h * w * c
    raw = np.frombuffer(bytes(rec), dtype=np.uint8)
    if records is None:
        records = raw.copy()
    else:
        records[:raw.size] = raw
    return packed, records, total, Cn, max(s[0] for s in shapes), max(s[1] for s in shapes)


def resize_u8_packed(src, src_bytes, samples, B, H, W, Cn, max_h, max_w, tables, out=None, check=False):
    """device half: `src` (uint8 device buffer holding the packed images), `samples` (uint8 device buffer holding B fp_resize_sample
    records) -> uint8 [B, H, W, C] -- the layout fp_assemble_images reads -- on the current launch stream.  The kernels turn down a
    record that points outside a buffer or names a table that does not fit its sizes and leave that sample unwritten; check=True reads
    the library's status word afterwards (this WAITS for the stream) and raises ValueError then -- for records the caller built itself;
    resize_pack's are right by construction."""
    lib = _lib.load()
    d_tables, n_tables, d_coeffs = tables.device_buffers()
    if out is None:
        out = torch.empty((B, H, W, Cn), dtype=torch.uint8, device=src.device)
    if out.numel() != B * H * W * Cn or out.dtype != torch.uint8 or src.dtype != torch.uint8 or src.numel() < src_bytes:
        raise RuntimeError("footprints_amd.ops.resize_u8_packed: out must be uint8 [B, H, W, C] and src hold src_bytes bytes")
    if samples.numel() * samples.element_size() < B * C.sizeof(_lib.ResizeSample):
        raise RuntimeError("footprints_amd.ops.resize_u8_packed: fewer than B sample records")
    need = lib.fp_resize_workspace(B, max_h, W, Cn)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.resize_u8_packed: bad sizes")
    ws = workspace(need, src.device, "resize")
    _lib.check(lib.fp_resize_u8(_chk(src, "src"), int(src_bytes), _chk(samples, "samples"), _chk(d_tables) if n_tables else None, n_tables,
                                _chk(d_coeffs) if n_tables else None, d_coeffs.numel() if n_tables else 0, _chk(out, "out"), B, H, W, Cn,
                                max_h, max_w, ws.data_ptr(), ws.numel(), stream()), "fp_resize_u8")
    if check:
        if _status_word(ws, lib.fp_resize_status_offset(B, max_h, W, Cn)) != 0:
            raise ValueError("footprints_amd.ops.resize_u8_packed: a sample or table record was turned down on the device; its output is unwritten")
    return out


def resize_u8(images, H, W, filter="lanczos", device="cuda"):
    """PIL.Image.resize((W, H), filter) of a batch of uint8 images of any (mixed) sizes, byte for byte, in one library call:
    images = list of numpy uint8 [h, w, 3], [h, w, 1] or [h, w] -> uint8 device tensor [B, H, W, C]"""
    tables = resize_table_set(device)
    packed, records, total, Cn, max_h, max_w = resize_pack(images, H, W, tables, filter)
    src = torch.from_numpy(packed).to(tables.device)
    rec = torch.from_numpy(records).to(tables.device)
    return resize_u8_packed(src, total, rec, len(images), H, W, Cn, max_h, max_w, tables)


def filter_depth_mask_workspace_bytes(B, H, W):
    n = _lib.load().fp_filter_depth_mask_workspace(B, H, W)
    if n < 0:
        raise RuntimeError("footprints_amd.ops.filter_depth_mask: B x H x W = %d x %d x %d is too large" % (B, H, W))
    return n


def filter_depth_mask(mask, out=None):
    """the reference's filter_depth_mask on the device: mask [B, H, W] or [H, W], float32 or float64 holding 0 / 1 -> same shape and type,
    1 on the 8-connected components of ones smaller than W * H / 100 pixels.  `out` may be `mask` (in place)."""
    if mask.dtype not in (torch.float32, torch.float64) or mask.dim() not in (2, 3):
        raise RuntimeError("footprints_amd.ops.filter_depth_mask: mask must be float32 or float64 [B, H, W] or [H, W]")
    H, W = mask.shape[-2:]
    B = mask.numel() // (H * W)
    out = torch.empty_like(mask) if out is None else out
    if out.shape != mask.shape or out.dtype != mask.dtype:
        raise RuntimeError("footprints_amd.ops.filter_depth_mask: out must match the mask")
    ws = workspace(filter_depth_mask_workspace_bytes(B, H, W), mask.device, "ccl")
    _lib.check(_lib.load().fp_filter_depth_mask(_chk(mask, "mask"), int(mask.dtype == torch.float64), _chk(out, "out"), B, H, W, ws.data_ptr(),
                                                ws.numel(), stream()), "fp_filter_depth_mask")
    return out


# ---- reader work on the device: the cv2 resizes of the label maps (csrc/label_resize.hip) ------------------------------------------------
LABEL_METHODS = {"zero": _lib.LABEL_ZERO, "nearest": _lib.LABEL_NEAREST, "area": _lib.LABEL_AREA, "pil_nearest": _lib.LABEL_PIL_NEAREST}
_area_host_tables = {}
_pil_nearest_axes = {}


def pil_nearest_axis(in_size, out_size):
    """the kernel's closed form of Pillow's NEAREST for one axis, min(floor((d + 0.5) * in / out), in - 1) -> int32 [out_size].  Pillow adds
    the step up in double (nearest_index restates that); where the two disagree -- a sum that lands a rounding error beside an integer --
    the axis is refused rather than resized almost like Pillow."""
    import numpy as np
    key = (int(in_size), int(out_size))
    idx = _pil_nearest_axes.get(key)
    if idx is None:
        d = np.arange(key[1], dtype=np.int64)
        idx = np.minimum((2 * d + 1) * key[0] // (2 * key[1]), key[0] - 1).astype(np.int32)
        if not np.array_equal(idx, nearest_index(*key)):
            raise ValueError("footprints_amd.ops.pil_nearest_axis: %d -> %d: Pillow's accumulated coordinate leaves the closed form" % key)
        idx.setflags(write=False)
        _pil_nearest_axes[key] = idx
    return idx


def area_table(in_size, out_size):
    """OpenCV's INTER_AREA table of one axis (computeResizeAreaTab), built by the library on the host (no GPU needed) and cached per
    (in, out) -> (bounds int32 [out, 2] = first entry and entry count of every output index, index int32 [n], weight float32 [n])"""
    import numpy as np
    key = (int(in_size), int(out_size))
    t = _area_host_tables.get(key)
    if t is None:
        lib = _lib.load()
        if key[0] <= 0 or key[1] <= 0 or key[1] > key[0]:
            raise ValueError("footprints_amd.ops.area_table: %d -> %d: sizes must be positive and INTER_AREA must not enlarge" % key)
        cap = key[0] + 2 * key[1]
        bounds, index, weight = np.empty((key[1], 2), np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32)
        n = lib.fp_area_table(key[0], key[1], bounds.ctypes.data, index.ctypes.data, weight.ctypes.data, cap)
        if n < 0:
            _lib.check(-1, "fp_area_table")
        index, weight = index[:n].copy(), weight[:n].copy()
        for a in (bounds, index, weight):
            a.setflags(write=False)
        t = _area_host_tables[key] = (bounds, index, weight)
    return t


class LabelTableSet(ResizeTableSet):
    """ResizeTableSet over INTER_AREA's tables: fp_label_table records over one buffer of 8-byte elements (uploaded as int64, bit for bit),
    a table's bounds one element per output index, its entries (int32 source index, float32 weight) one each"""

    def index(self, in_size, out_size):
        import numpy as np
        key = (int(in_size), int(out_size))
        with self.lock:
            i = self.keys.get(key)
            if i is None:
                bounds, idx, weight = area_table(*key)
                if int(bounds[:, 1].max()) > _lib.LABEL_MAX_ENTRIES:
                    raise ValueError("footprints_amd.ops: INTER_AREA %d -> %d needs %d entries per output, the kernel stages %d"
                                     % (key[0], key[1], int(bounds[:, 1].max()), _lib.LABEL_MAX_ENTRIES))
                entries = np.empty((idx.size, 2), np.int32)
                entries[:, 0] = idx
                entries[:, 1] = weight.view(np.int32)
                i = self.keys[key] = len(self.records)
                self.records.append(_lib.LabelTable(key[0], key[1], int(bounds[:, 1].max()), idx.size, self.length, self.length + key[1]))
                self.coeffs += [bounds.view(np.int64).reshape(-1), entries.view(np.int64).reshape(-1)]
                self.length += key[1] + idx.size
        return i


_label_table_sets = {}


def label_table_set(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _label_table_sets.get(device)
    if s is None:
        s = _label_table_sets[device] = LabelTableSet(device)
    return s


def _label_source(m):
    """a map as it is uploaded: the stored dtype when the kernel reads it (bool as uint8), float64 otherwise (.astype(float)) -> (array, FP_LABEL_*)"""
    import numpy as np
    m = np.asarray(m)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("footprints_amd.ops.label_resize_pack: a map must be a non-empty [h, w] array, got shape %r" % (m.shape,))
    if m.dtype == np.bool_:
        m = m.view(np.uint8)
    code = {np.dtype(np.uint8): _lib.LABEL_U8, np.dtype(np.float16): _lib.LABEL_F16, np.dtype(np.float32): _lib.LABEL_F32,
            np.dtype(np.float64): _lib.LABEL_F64, np.dtype(np.uint16): _lib.LABEL_U16}.get(m.dtype)
    if code is None:
        m, code = m.astype(np.float64), _lib.LABEL_F64
    return m, code


def label_source_itemsize(m):
    """bytes per element a map takes in the packed source buffer"""
    import numpy as np
    dt = np.asarray(m).dtype
    return dt.itemsize if dt in (np.dtype(np.bool_), np.dtype(np.uint8), np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.uint16)) else 8


def label_pack_bytes(maps):
    """bytes the maps (None = none) take in the packed source buffer, each padded to 8"""
    import numpy as np
    return sum((np.asarray(m).size * label_source_itemsize(m) + 7) // 8 * 8 for m in maps if m is not None)


def _per_map(v, n, name):
    if isinstance(v, (str, bool, int, float)) or getattr(v, "ndim", 1) == 0:
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError("footprints_amd.ops.label_resize_pack: %s must be one value or one per map" % name)
    return v


def label_area_fast(h, w, H, W):
    """whether cv2's INTER_AREA takes its integer path: both scales, computed as 1 / (out / in) in double, within DBL_EPSILON of an integer"""
    sx, sy = 1.0 / (float(W) / w), 1.0 / (float(H) / h)
    eps = 2.220446049250313e-16
    return abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps


def label_resize_pack(maps, H, W, method, flip=False, multiplier=1.0, tables=None, packed=None, records=None, max_map_hw=None):
    """host half of fp_label_resize: the maps ([h, w] arrays in the dtype the .npy holds; None = a map of zeros) one after the other at
    8-byte-aligned offsets of `packed` (a uint8 numpy buffer, e.g. pinned; allocated when None) and their fp_label_sample records in
    `records` (uint8 numpy view, allocated when None).  method ('zero' / 'nearest' / 'area', or 'pil_nearest': Pillow's resize(NEAREST),
    which is flipped after the resize, not before it), flip and multiplier: one value, or one per map.  uint16 maps are stored as they are.  tables: the LabelTableSet of the device (label_table_set).  INTER_AREA that would enlarge an axis is refused (cv2 switches to a
    linear kernel there, which is not provided), and so is a map larger than max_map_hw when that is given.
    -> (packed, records, bytes used, tables)"""
    import numpy as np
    n = len(maps)
    methods, flips, mults = _per_map(method, n, "method"), _per_map(flip, n, "flip"), _per_map(multiplier, n, "multiplier")
    if tables is None:
        tables = label_table_set("cuda")
    srcs, total = [], 0
    rec = (_lib.LabelSample * n)()
    for j, m in enumerate(maps):
        meth = LABEL_METHODS.get(methods[j], methods[j]) if isinstance(methods[j], str) else int(methods[j])
        if meth not in LABEL_METHODS.values():
            raise ValueError("footprints_amd.ops.label_resize_pack: method must be one of %s" % sorted(LABEL_METHODS))
        if m is None or meth == _lib.LABEL_ZERO:
            rec[j] = _lib.LabelSample(0, 0, 0, 0, _lib.LABEL_ZERO, 0, -1, -1, 0, 1.0)
            srcs.append(None)
            continue
        m, code = _label_source(m)
        h, w = m.shape
        if max_map_hw is not None and (h > max_map_hw[0] or w > max_map_hw[1]):
            raise ValueError("footprints_amd.ops.label_resize_pack: map %d is %d x %d, larger than max_map_hw = %r" % (j, h, w, tuple(max_map_hw)))
        tx = ty = -1
        if meth == _lib.LABEL_AREA and (h, w) != (H, W):
            if h < H or w < W:
                raise ValueError("footprints_amd.ops.label_resize_pack: map %d: INTER_AREA from %d x %d up to %d x %d is not provided "
                                 "(cv2 uses a linear kernel when it enlarges)" % (j, h, w, H, W))
            if not label_area_fast(h, w, H, W):
                tx, ty = tables.index(w, W), tables.index(h, H)
        if meth == _lib.LABEL_PIL_NEAREST:
            pil_nearest_axis(h, H), pil_nearest_axis(w, W)
        rec[j] = _lib.LabelSample(total, h, w, code, meth, int(bool(flips[j])), tx, ty, 0, float(mults[j]))
        srcs.append(m)
        total += (m.nbytes + 7) // 8 * 8
    if packed is None:
        packed = np.empty(max(total, 8), np.uint8)
    if total > packed.size:
        raise ValueError("footprints_amd.ops.label_resize_pack: the maps need %d source bytes, the buffer holds %d" % (total, packed.size))
    for r, m in zip(rec, srcs):
        if m is not None:
            np.copyto(packed[r.offset:r.offset + m.nbytes].view(m.dtype).reshape(m.shape), m)
    raw = np.frombuffer(bytes(rec), dtype=np.uint8)
    if records is None:
        records = raw.copy()
    else:
        records[:raw.size] = raw
    return packed, records, total, tables


def label_resize_packed(src, src_bytes, samples, n, H, W, tables, out=None, status=None, check=False):
    """device half: `src` (uint8 device buffer holding the packed maps), `samples` (uint8 device buffer holding n fp_label_sample records)
    -> float64 [n, H, W] (with n = K * B in map-major order: the [K, B, H, W] buffer fp_assemble_labels reads) on the current launch
    stream.  The kernel turns down a record that points outside the buffer or names a table that does not fit its sizes and leaves that
    map unwritten; check=True reads the status word afterwards (this WAITS for the stream) and raises ValueError then."""
    lib = _lib.load()
    d_tables, n_tables, d_entries = tables.device_buffers()
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.float64, device=src.device)
    if out.numel() != n * H * W or out.dtype != torch.float64 or src.dtype != torch.uint8 or src.numel() < src_bytes:
        raise RuntimeError("footprints_amd.ops.label_resize_packed: out must be float64 with n * H * W elements and src hold src_bytes bytes")
    if samples.numel() * samples.element_size() < n * C.sizeof(_lib.LabelSample):
        raise RuntimeError("footprints_amd.ops.label_resize_packed: fewer than n sample records")
    if status is None:
        status = workspace(4, src.device, "label_resize_status")[:4].view(torch.int32)
    _lib.check(lib.fp_label_resize(_chk(src, "src"), int(src_bytes), _chk(samples, "samples"), n, _chk(d_tables) if n_tables else None, n_tables,
                                   _chk(d_entries) if n_tables else None, d_entries.numel() if n_tables else 0,
                                   max((r.max_count for r in tables.records[:n_tables]), default=0), _chk(out, "out"), H, W,
                                   _chk(status, "status"), stream()), "fp_label_resize")
    if check and int(status.item()) != 0:
        raise ValueError("footprints_amd.ops.label_resize_packed: a sample or table record was turned down on the device; its map is unwritten")
    return out


def label_resize(maps, H, W, method, flip=False, multiplier=1.0, device="cuda"):
    """cv2.resize(m.astype(float), (W, H), interpolation=INTER_AREA | INTER_NEAREST) * multiplier of a list of maps of any (mixed) sizes
    and stored dtypes, bit for bit on float64, in one library call -> float64 device tensor [n, H, W].  With flip the result is
    cv2.resize(np.fliplr(m)) mirrored back -- what the assembler's own flip expects.  method 'pil_nearest' is
    Image.fromarray(m).resize((W, H), Image.NEAREST) instead (uint16 maps: mode I;16), flipped after the resize: mirrored back it is the
    unflipped resize."""
    tables = label_table_set(device)
    assert _lib.load().fp_label_sample_bytes() == C.sizeof(_lib.LabelSample) and _lib.load().fp_label_table_bytes() == C.sizeof(_lib.LabelTable)
    packed, records, total, _ = label_resize_pack(maps, H, W, method, flip, multiplier, tables)
    src = torch.from_numpy(packed).to(tables.device)
    rec = torch.from_numpy(records).to(tables.device)
    return label_resize_packed(src, total, rec, len(maps), H, W, tables, check=True)


# ---- loader work of the training-label generators on the device: cv2's resizes into a frame cache, batches out of it (csrc/gt_frames.hip) --
GT_METHODS = {"linear": _lib.GT_LINEAR, "nearest": _lib.GT_NEAREST, "area2": _lib.GT_AREA2}
_linear_host_tables = {}


def linear_table(in_size, out_size, clamp):
    """cv2's INTER_LINEAR offsets and float coefficients of one axis (fp_linear_table), built by the library on the host (no GPU needed)
    and cached per (in, out, clamp) -> (offsets int32 [out], coefficients float32 [out, 2]); clamp = the horizontal form"""
    import numpy as np
    key = (int(in_size), int(out_size), int(bool(clamp)))
    t = _linear_host_tables.get(key)
    if t is None:
        if key[0] <= 0 or key[1] <= 0:
            raise ValueError("footprints_amd.ops.linear_table: %d -> %d: sizes must be positive" % key[:2])
        offsets, coeffs = np.empty(key[1], np.int32), np.empty((key[1], 2), np.float32)
        _lib.check(_lib.load().fp_linear_table(key[0], key[1], key[2], offsets.ctypes.data, coeffs.ctypes.data), "fp_linear_table")
        for a in (offsets, coeffs):
            a.setflags(write=False)
        t = _linear_host_tables[key] = (offsets, coeffs)
    return t


class LinearTableSet(ResizeTableSet):
    """ResizeTableSet over INTER_LINEAR's tables: fp_gt_table records over one int32 buffer, a table's offsets first, then its coefficient bits"""

    def index(self, in_size, out_size, clamp):
        key = (int(in_size), int(out_size), int(bool(clamp)))
        with self.lock:
            i = self.keys.get(key)
            if i is None:
                import numpy as np
                offsets, coeffs = linear_table(*key)
                i = self.keys[key] = len(self.records)
                self.records.append(_lib.GtTable(key[0], key[1], key[2], self.length))
                self.coeffs += [offsets, coeffs.view(np.int32).reshape(-1)]
                self.length += 3 * key[1]
        return i

    def host_records(self):
        """(ctypes array of the fp_gt_table records or None, their count, length of the word buffer): what the host half validates against"""
        with self.lock:
            n = len(self.records)
            return ((_lib.GtTable * n)(*self.records) if n else None), n, self.length


_linear_table_sets = {}


def linear_table_set(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _linear_table_sets.get(device)
    if s is None:
        assert _lib.load().fp_gt_frame_bytes() == C.sizeof(_lib.GtFrame) and _lib.load().fp_gt_table_bytes() == C.sizeof(_lib.GtTable)
        s = _linear_table_sets[device] = LinearTableSet(device)
    return s


def _gt_source(m, pre, j):
    """a map as it is uploaded and its pre-scale as the kernel takes it: rounded to the stored dtype, like numpy's in-place `m *= pre`"""
    import numpy as np
    m = np.asarray(m)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("footprints_amd.ops.gt_frame_pack: map %d must be a non-empty [h, w] array, got shape %r" % (j, m.shape))
    code = {np.dtype(np.float16): _lib.GT_F16, np.dtype(np.float32): _lib.GT_F32, np.dtype(np.float64): _lib.GT_F64,
            np.dtype(np.uint16): _lib.GT_U16}.get(m.dtype)
    if code is None:
        if m.dtype.kind not in "bui" or m.dtype.itemsize > 4:
            raise ValueError("footprints_amd.ops.gt_frame_pack: map %d: dtype %s is not provided" % (j, m.dtype))
        m, code = m.astype(np.float64), _lib.GT_F64                # .astype(float) is exact for these; numpy refuses to pre-scale them in place
        if float(pre) != 1.0:
            raise ValueError("footprints_amd.ops.gt_frame_pack: map %d: an integer map takes no pre-scale" % j)
    if code == _lib.GT_U16:
        if float(pre) != 1.0:
            raise ValueError("footprints_amd.ops.gt_frame_pack: map %d: an integer map takes no pre-scale" % j)
        return m, code, 1.0
    return m, code, float(m.dtype.type(pre))


def gt_frame_pack_bytes(maps):
    """bytes that `maps` and their records take in the packed buffer of gt_frame_pack"""
    import numpy as np
    total = 0
    for m in maps:
        m = np.asarray(m)
        item = m.dtype.itemsize if m.dtype in (np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.uint16)) else 8
        total += (m.size * item + 7) // 8 * 8
    return total + len(maps) * C.sizeof(_lib.GtFrame)


class GtFramePack:
    """what gt_frame_pack hands to gt_frame_resize: `packed` (uint8 numpy buffer, possibly pinned) holds the maps in [0, src_bytes) and the
    n fp_gt_frame records in [records_offset, total); `records` is the validated host copy of the latter"""

    def __init__(self, packed, src_bytes, records_offset, total, records, n, H, W, cache_elems, tables):
        self.packed, self.src_bytes, self.records_offset, self.total = packed, src_bytes, records_offset, total
        self.records, self.n, self.H, self.W, self.cache_elems, self.tables = records, n, H, W, cache_elems, tables


def gt_frame_pack(maps, H, W, dst, cache_elems, method="linear", pre=1.0, post=1.0, threshold=None, tables=None, packed=None):
    """host half of fp_gt_frame_resize (no GPU needed): the maps ([h, w] arrays in the dtype the .npy holds: float16 / float32 / float64 /
    uint16) one after the other at 8-byte-aligned offsets of `packed` (a uint8 numpy buffer, e.g. pinned; allocated when None), their
    fp_gt_frame records behind them, and the records validated against the packed bytes, a cache of `cache_elems` float32 elements and the
    tables (ValueError names the first bad one).  dst: each map's element offset into the cache (slot * H * W).  method ('linear' /
    'nearest' / 'area2'), pre, post (a factor, or (numerator, denominator): the value is (v * numerator) / denominator) and threshold (None
    = none): one value, or one per map.  'linear' at exactly twice the target on both axes is dispatched to 'area2', as cv::resize does.
    tables: the LinearTableSet of the device.  -> GtFramePack"""
    import numpy as np
    n = len(maps)
    if n == 0:
        raise ValueError("footprints_amd.ops.gt_frame_pack: no maps")
    lib = _lib.load()
    per = lambda v, name: [v] * n if (v is None or isinstance(v, (str, int, float, tuple)) or getattr(v, "ndim", 1) == 0) else _per_map(v, n, name)
    methods, pres, posts, thrs, dsts = per(method, "method"), per(pre, "pre"), per(post, "post"), per(threshold, "threshold"), _per_map(dst, n, "dst")
    if tables is None:
        tables = linear_table_set("cuda")
    rec = (_lib.GtFrame * n)()
    srcs, total = [], 0
    for j, m in enumerate(maps):
        meth = GT_METHODS.get(methods[j], methods[j]) if isinstance(methods[j], str) else int(methods[j])
        if meth not in GT_METHODS.values():
            raise ValueError("footprints_amd.ops.gt_frame_pack: method must be one of %s" % sorted(GT_METHODS))
        m, code, p = _gt_source(m, pres[j], j)
        h, w = m.shape
        if meth == _lib.GT_LINEAR and label_area_fast(h, w, H, W) and round(1.0 / (float(W) / w)) == 2 and round(1.0 / (float(H) / h)) == 2:
            meth = _lib.GT_AREA2                                     # cv::resize: INTER_LINEAR with both integer scales 2 becomes INTER_AREA
        tx = ty = -1
        if meth == _lib.GT_LINEAR:
            tx, ty = tables.index(w, W, True), tables.index(h, H, False)
        num, den = posts[j] if isinstance(posts[j], tuple) else (posts[j], 1.0)
        thr = thrs[j]
        rec[j] = _lib.GtFrame(total, int(dsts[j]), h, w, code, meth, tx, ty, int(thr is not None), 0, p, float(num), float(den),
                              0.0 if thr is None else float(thr))
        srcs.append(m)
        total += (m.nbytes + 7) // 8 * 8
    src_bytes, total = total, total + n * C.sizeof(_lib.GtFrame)
    t_rec, n_tables, words_len = tables.host_records()
    if lib.fp_gt_frame_check(C.addressof(rec), n, src_bytes, C.addressof(t_rec) if n_tables else None, n_tables, words_len, int(cache_elems), H, W):
        msg = lib.fp_last_error_string()
        raise ValueError("footprints_amd.ops.gt_frame_pack: %s" % (msg.decode() if msg else "?"))
    if packed is None:
        packed = np.empty(total, np.uint8)
    if total > packed.size:
        raise ValueError("footprints_amd.ops.gt_frame_pack: the maps and records need %d bytes, the buffer holds %d" % (total, packed.size))
    for r, m in zip(rec, srcs):
        np.copyto(packed[r.offset:r.offset + m.nbytes].view(m.dtype).reshape(m.shape), m)
    packed[src_bytes:total] = np.frombuffer(bytes(rec), dtype=np.uint8)
    return GtFramePack(packed, src_bytes, src_bytes, total, rec, n, H, W, int(cache_elems), tables)


def gt_frame_resize(pack, d_packed, cache):
    """device half: d_packed (uint8 device buffer holding pack.packed[:pack.total]) -> every map resized into its slot of `cache` (float32
    device tensor of pack.cache_elems elements) on the current launch stream, one launch.  The library validates pack.records once more
    before it launches; Python sees ValueError."""
    lib = _lib.load()
    if d_packed.dtype != torch.uint8 or d_packed.numel() < pack.total or cache.dtype != torch.float32 or cache.numel() != pack.cache_elems:
        raise RuntimeError("footprints_amd.ops.gt_frame_resize: d_packed must be uint8 and hold pack.total bytes, cache float32 of pack.cache_elems elements")
    d_tables, n_tables, d_words = pack.tables.device_buffers()
    t_rec, n_host, words_len = pack.tables.host_records()
    n_tables = min(n_tables, n_host)
    base = _chk(d_packed, "d_packed")
    rc = lib.fp_gt_frame_resize(base, pack.src_bytes, C.addressof(pack.records), base + pack.records_offset, pack.n,
                                C.addressof(t_rec) if n_tables else None, _chk(d_tables) if n_tables else None, n_tables,
                                _chk(d_words) if n_tables else None, d_words.numel() if n_tables else 0, _f32(cache, "cache"), cache.numel(),
                                pack.H, pack.W, stream())
    if rc == -1:                                                     # FP_EINVAL: a record was turned down, nothing was launched
        msg = lib.fp_last_error_string()
        raise ValueError("footprints_amd.ops.gt_frame_resize: %s" % (msg.decode() if msg else "?"))
    _lib.check(rc, "fp_gt_frame_resize")
    return cache


def gt_frames(maps, H, W, method="linear", pre=1.0, post=1.0, threshold=None, device="cuda"):
    """the resizes of the label generators' loader for a list of maps of any (mixed) sizes and stored dtypes, in one library call -> float32
    device tensor [n, H, W] (a cache of its own, map j in slot j)"""
    tables = linear_table_set(device)
    cache = torch.empty((len(maps), H, W), dtype=torch.float32, device=tables.device)
    pack = gt_frame_pack(maps, H, W, [j * H * W for j in range(len(maps))], cache.numel(), method, pre, post, threshold, tables)
    return gt_frame_resize(pack, torch.from_numpy(pack.packed[:pack.total]).to(tables.device), cache)


def gt_gather_frames(cache, depth_slots, seg_slots, fb=None):
    """the batch of one target frame out of a frame cache (float32 [n_slots, H, W]): depths[b] = fb / cache[depth_slots[b]] (IEEE float32
    division; fb = the float32 fx * baseline) or, with fb None, the slot itself; ground_segs[b] = cache[seg_slots[b]].  Slots may repeat and
    come in any order; one outside the cache raises ValueError before anything is launched.  -> (depths, ground_segs) float32 [B, H, W]"""
    import numpy as np
    if cache.dim() != 3:
        raise RuntimeError("footprints_amd.ops.gt_gather_frames: the cache must be [n_slots, H, W]")
    n_slots, H, W = cache.shape
    slots = np.ascontiguousarray(np.stack([np.asarray(depth_slots, np.int64).reshape(-1), np.asarray(seg_slots, np.int64).reshape(-1)]))
    B = slots.shape[1]
    if B == 0 or slots.min() < 0 or slots.max() >= n_slots:
        raise ValueError("footprints_amd.ops.gt_gather_frames: %d frames with slots %s .. %s, the cache holds %d slots"
                         % (B, slots.min() if B else None, slots.max() if B else None, n_slots))
    slots = slots.astype(np.int32)
    c = _f32(cache, "cache")
    d_slots = torch.from_numpy(slots).to(cache.device)
    depths = torch.empty((B, H, W), dtype=torch.float32, device=cache.device)
    ground_segs = torch.empty((B, H, W), dtype=torch.float32, device=cache.device)
    _lib.check(_lib.load().fp_gt_gather_frames(c, n_slots, slots.ctypes.data, _chk(d_slots), B, H, W, int(fb is not None),
                                               0.0 if fb is None else float(fb), _chk(depths), _chk(ground_segs), stream()), "fp_gt_gather_frames")
    return depths, ground_segs


def to_tensor_u8(images_hwc):
    """ToTensor on the device: uint8 [B, H, W, 3] -> float32 [B, 3, H, W] in [0, 1] (fp_assemble_images without flip or jitter)"""
    B, H, W, Cn = images_hwc.shape
    if Cn != 3 or images_hwc.dtype != torch.uint8:
        raise RuntimeError("footprints_amd.ops.to_tensor_u8: images must be uint8 [B, H, W, 3]")
    dev = images_hwc.device
    params = torch.zeros(B * _lib.load().fp_aug_params_bytes(), dtype=torch.uint8, device=dev)        # flip = 0, n_ops = 0
    sums = torch.empty(B, dtype=torch.int64, device=dev)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().fp_assemble_images(_chk(images_hwc, "images"), _chk(params), _chk(sums), _chk(out), B, H, W, stream()), "fp_assemble_images")
    return out


def load_images_u8(images, H, W, filter="lanczos", device="cuda"):
    """Resize((H, W)) + ToTensor of decoded RGB frames (numpy uint8 [h, w, 3], any sizes) on the device: one upload of the raw bytes
    -> float32 [B, 3, H, W], bit-equal to PIL's resize followed by a division by 255 in float32"""
    return to_tensor_u8(resize_u8(images, H, W, filter, device))


# ---- reader work of the segmentation trainer: windowed per-sample resize and the label path (csrc/resample_u8.hip, csrc/seg_reader.hip) ----------
def resize_tables_range(in_size, out_size, first, count, filter="lanczos"):
    """rows first .. first + count - 1 of `resize_tables(in_size, out_size, filter)`, built alone: the cost is that of `count` rows.  Not
    cached -- the segmentation reader's target sizes are random per sample."""
    import numpy as np
    lib = _lib.load()
    key = (int(in_size), int(out_size), _resize_filter(filter))
    ksize = lib.fp_resize_ksize(*key)
    if ksize < 0:
        raise ValueError("footprints_amd.ops.resize_tables_range: bad sizes %r" % (key,))
    bounds, kk = np.empty((count, 2), np.int32), np.empty((count, ksize), np.int32)
    _lib.check(lib.fp_resize_coeffs_range(key[0], key[1], key[2], int(first), int(count), bounds.ctypes.data, kk.ctypes.data, ksize),
               "fp_resize_coeffs_range")
    return bounds, kk


def nearest_index(in_size, out_size):
    """source index of every output index of Pillow's NEAREST resize of one axis -> int32 [out_size]"""
    import numpy as np
    idx = np.empty(int(out_size), np.int32)
    _lib.check(_lib.load().fp_nearest_index(int(in_size), int(out_size), idx.ctypes.data), "fp_nearest_index")
    return idx


def resize_window_axis(in_size, out_size, first, count, filter="lanczos", whole_table=False):
    """one axis of a windowed resize on the host -> (table, lo, hi): table = None when the sizes agree (the pass is skipped), else
    (first row described, bounds, kk) for the window's output indices (or for all of them with whole_table); [lo, hi) = the source
    indices the window's taps reach"""
    if first < 0 or count <= 0 or first + count > out_size:
        raise ValueError("footprints_amd.ops.resize_window_axis: the window %d + %d leaves the target size %d" % (first, count, out_size))
    if in_size == out_size:
        return None, first, first + count
    t0, n = (0, out_size) if whole_table else (first, count)
    bounds, kk = resize_tables_range(in_size, out_size, t0, n, filter)
    w = bounds[first - t0:first - t0 + count]
    return (t0, bounds, kk), int(w[:, 0].min()), int((w[:, 0] + w[:, 1]).max())


class WindowBatch:
    """host half of one fp_resize_window_u8 call: the sample records, table records and coefficient rows, collected sample by sample"""

    def __init__(self, channels=3):
        self.C = int(channels)
        self.samples, self.tables, self.coeffs, self.length = [], [], [], 0
        self.max_src_h = self.max_src_w = self.max_win_h = self.max_win_w = 1

    def table(self, in_size, out_size, t):
        """index of the table `t` of resize_window_axis in this call's table list; -1 for None"""
        if t is None:
            return -1
        first, bounds, kk = t
        self.tables.append(_lib.ResizeWindowTable(in_size, out_size, kk.shape[1], first, bounds.shape[0], self.length, self.length + bounds.size))
        self.coeffs += [bounds.reshape(-1), kk.reshape(-1)]
        self.length += bounds.size + kk.size
        return len(self.tables) - 1

    def add(self, src_offset, rect, table_h, table_v, window, out_offset):
        """rect = (y0, x0, h, w) of the staged source rectangle in its image, window = (top, left, h, w) of the target"""
        y0, x0, h, w = (int(v) for v in rect)
        top, left, wh, ww = (int(v) for v in window)
        self.samples.append(_lib.ResizeWindowSample(int(src_offset), int(out_offset), h, w, y0, x0, table_h, table_v, top, left, wh, ww))
        self.max_src_h, self.max_src_w = max(self.max_src_h, h), max(self.max_src_w, w)
        self.max_win_h, self.max_win_w = max(self.max_win_h, wh), max(self.max_win_w, ww)

    def arrays(self):
        """(sample records uint8, table records uint8, coefficients int32) as numpy arrays"""
        import numpy as np
        rec = np.frombuffer(b"".join(bytes(r) for r in self.samples), dtype=np.uint8)
        tab = np.frombuffer(b"".join(bytes(r) for r in self.tables), dtype=np.uint8)
        return rec, tab, (np.concatenate(self.coeffs) if self.coeffs else np.zeros(0, np.int32))


def resize_window_u8(src, src_bytes, samples, B, tables, n_tables, coeffs, coeffs_len, out, Cn, max_src_h, max_src_w, max_win_h, max_win_w,
                     check=False):
    """device half of a windowed resize (fp_resize_window_u8) on the current launch stream: src / out uint8 device buffers, samples B
    fp_resize_window_sample records, tables n_tables fp_resize_window_table records over the int32 buffer `coeffs` -- all on the device.
    Per sample the bytes of Image.resize(its target size).crop(its window) land at its out_offset.  check=True reads the status word
    afterwards (this WAITS for the stream) and raises ValueError when a record was turned down."""
    lib = _lib.load()
    if src.dtype != torch.uint8 or out.dtype != torch.uint8 or src.numel() < src_bytes:
        raise RuntimeError("footprints_amd.ops.resize_window_u8: src and out must be uint8 and src hold src_bytes bytes")
    if samples.numel() * samples.element_size() < B * C.sizeof(_lib.ResizeWindowSample):
        raise RuntimeError("footprints_amd.ops.resize_window_u8: fewer than B sample records")
    if n_tables and (tables.numel() * tables.element_size() < n_tables * C.sizeof(_lib.ResizeWindowTable) or coeffs.dtype != torch.int32
                     or coeffs.numel() < coeffs_len):
        raise RuntimeError("footprints_amd.ops.resize_window_u8: fewer than n_tables table records, or coeffs is not int32 of coeffs_len")
    need = lib.fp_resize_window_workspace(B, max_src_h, max_win_w, Cn)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.resize_window_u8: bad sizes")
    ws = workspace(need, src.device, "resize_window")
    _lib.check(lib.fp_resize_window_u8(_chk(src, "src"), int(src_bytes), _chk(samples, "samples"), _chk(tables, "tables") if n_tables else None,
                                       n_tables, _chk(coeffs, "coeffs") if n_tables else None, int(coeffs_len) if n_tables else 0, _chk(out, "out"),
                                       out.numel(), B, Cn, max_src_h, max_src_w, max_win_h, max_win_w, ws.data_ptr(), ws.numel(), stream()),
               "fp_resize_window_u8")
    if check:
        if _status_word(ws, lib.fp_resize_window_status_offset(B, max_src_h, max_win_w, Cn)) != 0:
            raise ValueError("footprints_amd.ops.resize_window_u8: a sample or table record was turned down on the device; its output is unwritten")
    return out


def resize_window_status(device, B, max_src_h, max_win_w, Cn):
    """the status word the last resize_window_u8 call of these sizes on the current stream left (WAITS for the stream)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    off = _lib.load().fp_resize_window_status_offset(B, max_src_h, max_win_w, Cn)
    return _status_word(workspace(off + 16, device, "resize_window"), off)


def seg_labels(src, src_bytes, samples, B, index, index_len, ground_ids, set_offsets, H, W, ground_mask=None, labelled_pix=None, status=None,
               check=False):
    """fp_seg_labels on the current launch stream: src uint8 device buffer with the staged label rectangles, samples B fp_seg_label_sample
    records, index the int32 row / column tables, ground_ids / set_offsets the int32 ground-id sets -- all on the device
    -> (ground_mask, labelled_pix) float32 [B, H, W]"""
    dev = src.device
    if src.dtype != torch.uint8 or index.dtype != torch.int32 or ground_ids.dtype != torch.int32 or set_offsets.dtype != torch.int32:
        raise RuntimeError("footprints_amd.ops.seg_labels: src must be uint8; index, ground_ids and set_offsets int32")
    if samples.numel() * samples.element_size() < B * C.sizeof(_lib.SegLabelSample) or src.numel() < src_bytes or index.numel() < index_len:
        raise RuntimeError("footprints_amd.ops.seg_labels: fewer than B sample records, src_bytes source bytes or index_len table entries")
    ground_mask = torch.empty((B, H, W), dtype=torch.float32, device=dev) if ground_mask is None else ground_mask
    labelled_pix = torch.empty((B, H, W), dtype=torch.float32, device=dev) if labelled_pix is None else labelled_pix
    status = torch.empty(1, dtype=torch.int32, device=dev) if status is None else status
    if ground_mask.numel() != B * H * W or labelled_pix.numel() != B * H * W or status.dtype != torch.int32:
        raise RuntimeError("footprints_amd.ops.seg_labels: outputs must be float32 [B, H, W] and status one int32")
    _lib.check(_lib.load().fp_seg_labels(_chk(src, "src"), int(src_bytes), _chk(samples, "samples"), _chk(index, "index"), int(index_len),
                                         _chk(ground_ids, "ground_ids"), ground_ids.numel(), _chk(set_offsets, "set_offsets"),
                                         set_offsets.numel() - 1, _f32(ground_mask, "ground_mask"), _f32(labelled_pix, "labelled_pix"),
                                         _chk(status, "status"), B, H, W, stream()), "fp_seg_labels")
    if check and int(status.item()) != 0:
        raise ValueError("footprints_amd.ops.seg_labels: a sample record or a table entry was turned down on the device")
    return ground_mask, labelled_pix


# ---- visualisations on the device: predict_simple's overlay and the test-set side-by-side picture (csrc/visualise.hip) -----------------------
_vis_host_tables = {}


def vis_tables(in_size, out_size, filter="bilinear"):
    """the tables of `resize_tables` before the quantisation, as Pillow's mode-"F" passes use them, cached per (in, out, filter)
    -> (bounds int32 [out, 2], kk float64 [out, ksize] = the taps normalised in double)"""
    import numpy as np
    key = (int(in_size), int(out_size), _resize_filter(filter))
    t = _vis_host_tables.get(key)
    if t is None:
        lib = _lib.load()
        ksize = lib.fp_resize_ksize(*key)
        if ksize < 0:
            raise ValueError("footprints_amd.ops.vis_tables: bad sizes %r" % (key,))
        bounds, kk = np.empty((key[1], 2), np.int32), np.empty((key[1], ksize), np.float64)
        _lib.check(lib.fp_resize_coeffs_f64(key[0], key[1], key[2], bounds.ctypes.data, kk.ctypes.data, ksize), "fp_resize_coeffs_f64")
        bounds.setflags(write=False)
        kk.setflags(write=False)
        t = _vis_host_tables[key] = (bounds, kk)
    return t


class VisTableSet(ResizeTableSet):
    """ResizeTableSet over the double tables: one buffer of 8-byte elements (uploaded as int64, bit for bit) in which a table's bounds take
    one element per output index and its taps one each; offsets count those elements"""

    def index(self, in_size, out_size, filter="bilinear"):
        return super().index(in_size, out_size, filter)

    def _host_tables(self, key):
        import numpy as np
        bounds, kk = vis_tables(*key)
        return bounds.view(np.int64).reshape(-1), kk.view(np.int64).reshape(-1), kk.shape[1]


_vis_table_sets = {}
_vis_luts = {}


def vis_table_set(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _vis_table_sets.get(device)
    if s is None:
        assert _lib.load().fp_resize_table_bytes() == C.sizeof(_lib.ResizeTable) and _lib.load().fp_resize_sample_bytes() == C.sizeof(_lib.ResizeSample)
        s = _vis_table_sets[device] = VisTableSet(device)
    return s


def vis_colour_table():
    """uint8 [256, 3] numpy: matplotlib's plasma map with 256 entries, `(rgba[:, :3] * 255).astype(uint8)`, read at first use"""
    import numpy as np
    lut = _vis_luts.get("host")
    if lut is None:
        import matplotlib
        # what matplotlib.pyplot.get_cmap("plasma", 256) returns, without importing pyplot or touching the caller's backend
        rgba = matplotlib.colormaps["plasma"].resampled(256)(np.arange(256))
        lut = _vis_luts["host"] = np.ascontiguousarray((rgba[:, :3] * 255).astype(np.uint8))
        lut.setflags(write=False)
    return lut


def _vis_lut(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = _vis_luts.get(device)
    if t is None:
        t = _vis_luts[device] = torch.from_numpy(vis_colour_table().copy()).to(device)
    return t


def vis_records(shapes, H, W, tables):
    """fp_resize_sample records of photos of `shapes` = [(h, w), ...] lying one after the other in a packed buffer, for a prediction of
    H x W -> (records uint8 numpy, bytes of the packed buffer, max_h, max_w)"""
    import numpy as np
    rec = (_lib.ResizeSample * len(shapes))()
    off = 0
    for b, (h, w) in enumerate(shapes):
        rec[b] = _lib.ResizeSample(off, h, w, tables.index(W, w), tables.index(H, h))
        off += h * w * 3
    return np.frombuffer(bytes(rec), dtype=np.uint8).copy(), off, max(s[0] for s in shapes), max(s[1] for s in shapes)


def vis_overlay_packed(pred, src, src_bytes, samples, max_h, max_w, tables, out=None, check=False):
    """device half of the overlay: pred float32 [B, 4, H, W], `src` the packed photos (uint8 device buffer, src_bytes used), `samples`
    B fp_resize_sample records on the device (vis_records) -> uint8 device buffer with the photos' layout.  check=True reads the
    library's status word afterwards (this WAITS for the stream) and raises ValueError when a record was turned down."""
    lib = _lib.load()
    if pred.dim() != 4 or pred.shape[1] != 4:
        raise RuntimeError("footprints_amd.ops.vis_overlay_packed: pred must be float32 [B, 4, H, W]")
    B, _, H, W = pred.shape
    d_tables, n_tables, d_coeffs = tables.device_buffers()
    if out is None:
        out = torch.empty(int(src_bytes), dtype=torch.uint8, device=pred.device)
    if out.dtype != torch.uint8 or src.dtype != torch.uint8 or src.numel() < src_bytes or out.numel() < src_bytes:
        raise RuntimeError("footprints_amd.ops.vis_overlay_packed: src and out must be uint8 buffers of at least src_bytes bytes")
    if samples.numel() * samples.element_size() < B * C.sizeof(_lib.ResizeSample):
        raise RuntimeError("footprints_amd.ops.vis_overlay_packed: fewer than B sample records")
    need = lib.fp_vis_overlay_workspace(B, H, W, max_h, max_w)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.vis_overlay_packed: bad sizes, or too large")
    ws = workspace(need, pred.device, "vis")
    _lib.check(lib.fp_vis_overlay(_f32(pred, "pred"), _chk(src, "src"), int(src_bytes), _chk(samples, "samples"), _chk(d_tables) if n_tables else None,
                                  n_tables, _chk(d_coeffs) if n_tables else None, d_coeffs.numel() if n_tables else 0, _chk(_vis_lut(pred.device)),
                                  _chk(out, "out"), B, H, W, max_h, max_w, ws.data_ptr(), ws.numel(), stream()), "fp_vis_overlay")
    if check:
        off = lib.fp_vis_overlay_status_offset(B, H, W, max_h, max_w)
        if int(ws[off:off + 4].view(torch.int32).item()) != 0:
            raise ValueError("footprints_amd.ops.vis_overlay_packed: a sample or table record was turned down on the device; its output is unwritten")
    return out


def vis_overlay(pred, originals=None, packed=None, shapes=None):
    """predict_simple.InferenceManager.visualise for a batch, byte for byte, in one library call and one copy to the host:
    pred float32 device [B, 4, H, W]; the photos either as `originals` (list of numpy uint8 [h, w, 3] of any sizes, uploaded here) or, when
    they are on the device already (the buffer resize_pack filled, uploaded for the device resize), as `packed` + `shapes` = their
    (h, w) in the buffer's order -> list of B numpy uint8 [h, w, 3]"""
    out, total, shapes = vis_overlay_device(pred, originals, packed, shapes)
    return split_pictures(out[:total].cpu().numpy(), shapes)


def split_pictures(host, shapes):
    """views [h, w, 3] of pictures lying one after the other in a packed uint8 numpy buffer"""
    views, off = [], 0
    for h, w in shapes:
        views.append(host[off:off + h * w * 3].reshape(h, w, 3))
        off += h * w * 3
    return views


def vis_overlay_device(pred, originals=None, packed=None, shapes=None):
    """vis_overlay without the copy to the host -> (uint8 device buffer, its bytes in use, the (h, w) of the overlays lying in it one
    after the other): what jpeg_encode_packed takes with jpeg_records of the same shapes"""
    import numpy as np
    B, H, W = pred.shape[0], pred.shape[2], pred.shape[3]
    if (originals is None) == (packed is None) or (packed is not None and shapes is None):
        raise ValueError("footprints_amd.ops.vis_overlay: pass either originals, or packed and shapes")
    if originals is not None:
        if any(im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 for im in originals):
            raise ValueError("footprints_amd.ops.vis_overlay: originals must be uint8 [h, w, 3]")
        shapes = [im.shape[:2] for im in originals]
    shapes = [(int(h), int(w)) for h, w in shapes]
    if len(shapes) != B:
        raise ValueError("footprints_amd.ops.vis_overlay: %d predictions, %d photos" % (B, len(shapes)))
    tables = vis_table_set(pred.device)
    records, total, max_h, max_w = vis_records(shapes, H, W, tables)
    if originals is not None:
        packed = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in originals])).to(pred.device)
    return vis_overlay_packed(pred, packed, total, torch.from_numpy(records).to(pred.device), max_h, max_w, tables), total, shapes


def vis_side_by_side(image, pred, out=None):
    """the test-set picture (reference evaluation/inference.py:114-118): image float32 [B, 3, H, W] in [0, 1] and the logits pred
    [B, 4, H, W] -> uint8 device tensor [B, H, 2 W, 3], the image as bytes beside the mask channel in the colour table's first and last colour"""
    B, _, H, W = pred.shape
    if tuple(image.shape) != (B, 3, H, W) or pred.shape[1] != 4:
        raise RuntimeError("footprints_amd.ops.vis_side_by_side: image must be [B, 3, H, W] and pred [B, 4, H, W]")
    if out is None:
        out = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device=pred.device)
    lut = vis_colour_table()
    colour = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
    _lib.check(_lib.load().fp_vis_side_by_side(_f32(image, "image"), _f32(pred, "pred"), _chk(out, "out"), B, H, W, colour(lut[0]), colour(lut[255]),
                                               stream()), "fp_vis_side_by_side")
    return out


# ---- the trainer's TensorBoard pictures (csrc/log_panels.hip) ---------------------------------------------------------------------------------
LOG_PANEL_TAGS = ("image", "target_disp", "target_visible_ground", "target_all_ground", "target_ground_depth", "depth_mask", "moving_pixels",
                  "pred_disp_1", "pred_ground_visible_1", "pred_ground_all_1", "pred_ground_disp_1", "pred_ground_disp_masked_1")
_log_workspaces = {}
_LOG_LABELS = ("visible_ground", "depth", "ground_depth", "moving_object_mask", "depth_mask", "all_ground")      # fp_log_panels' argument order


def log_panel_tags(n, moving=True):
    """the tags of the reference's log (training/logger.py:19-67) in the order it writes them: sample by sample, panel by panel"""
    return ["%s/%d" % (t, i) for i in range(n) for t in LOG_PANEL_TAGS if moving or t != "moving_pixels"]


def log_panels(inputs, pred, depth_range, n=4, out=None):
    """the pictures of one log event for the first min(n, B) samples, in two launches on the current stream: inputs = the batch (image
    float32 [B, 3, H, W] and the label maps [B, H, W] or [B, 1, H, W]; 'moving_object_mask' may be missing or None, as in the reference),
    pred = the raw scale-1/1 output [B, 4, H, W] -> (uint8 device tensor [n, P, H, W, 3], the n * P tags in the tensor's order)"""
    lib = _lib.load()
    image = inputs["image"]
    if image.dim() != 4 or image.shape[1] != 3 or pred.dim() != 4 or pred.shape[1] != 4 or pred.shape[0] != image.shape[0] or \
            pred.shape[2:] != image.shape[2:]:
        raise RuntimeError("footprints_amd.ops.log_panels: image must be [B, 3, H, W] and pred [B, 4, H, W]")
    B, _, H, W = image.shape
    n = min(int(n), B)
    labels = []
    for key in _LOG_LABELS:
        t = inputs.get(key)
        if t is None and key != "moving_object_mask":
            raise RuntimeError("footprints_amd.ops.log_panels: the batch has no %r" % key)
        if t is not None and t.numel() != B * H * W:
            raise RuntimeError("footprints_amd.ops.log_panels: %s must be [B, H, W] or [B, 1, H, W]" % key)
        labels.append(t)
    P = 12 if labels[3] is not None else 11
    if out is None:
        out = torch.empty((n, P, H, W, 3), dtype=torch.uint8, device=pred.device)
    if out.dtype != torch.uint8 or out.numel() != n * P * H * W * 3:
        raise RuntimeError("footprints_amd.ops.log_panels: out must be uint8 [%d, %d, %d, %d, 3]" % (n, P, H, W))
    need = lib.fp_log_panels_workspace(n, H, W)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.log_panels: bad sizes, or too large")
    # a buffer of its own, not ops.workspace: no recorded launch plan holds its address, so its allocation must not make TrainStep drop them
    key = (pred.device.index, stream())
    ws = _log_workspaces.get(key)
    if ws is None or ws.numel() < need:
        release(ws, "workspace:log_panels")
        ws = _log_workspaces[key] = torch.empty(int(need), dtype=torch.uint8, device=pred.device)
    _lib.check(lib.fp_log_panels(_f32(image, "image"), *[_f32(t, k) if t is not None else None for t, k in zip(labels, _LOG_LABELS)],
                                 _f32(pred, "pred"), _chk(_vis_lut(pred.device)), _chk(out, "out"), B, n, H, W, float(depth_range[0]),
                                 float(depth_range[1]), ws.data_ptr(), ws.numel(), stream()), "fp_log_panels")
    return out.view(n, P, H, W, 3), log_panel_tags(n, moving=P == 12)


# ---- stretched maps as pictures (csrc/stretch_map.hip) ----------------------------------------------------------------------------------------
_colour_tables = {}
_stretch_workspaces = {}


def colour_table(name, rule):
    """uint8 [256, 3] numpy, read-only: the 256 colours of matplotlib's map `name` as bytes, read from matplotlib at first use.
    rule "bytes": `(cmap(arange(256))[:, :3] * 255).astype(uint8)` in float64, matplotlib's own table for `bytes=True` (imsave);
    rule "float32": `(float32(colour) * 255).astype(uint8)`, what tensorboardX makes of the float colours a log hands it"""
    import numpy as np
    key = (str(name), str(rule))
    lut = _colour_tables.get(key)
    if lut is None:
        if rule not in ("bytes", "float32"):
            raise ValueError("footprints_amd.ops.colour_table: rule must be 'bytes' or 'float32'")
        import matplotlib
        rgb = matplotlib.colormaps[name].resampled(256)(np.arange(256))[:, :3]
        if rule == "float32":
            rgb = rgb.astype(np.float32) * np.float32(255)
        else:
            rgb = rgb * 255
        lut = _colour_tables[key] = np.ascontiguousarray(rgb.astype(np.uint8))
        lut.setflags(write=False)
    return lut


def _colour_lut(name, rule, device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(name), str(rule), device)
    t = _colour_tables.get(key)
    if t is None:
        t = _colour_tables[key] = torch.from_numpy(colour_table(name, rule).copy()).to(device)
    return t


def _own_workspace(cache, tag, need, device):
    """a buffer of its own, not ops.workspace: no recorded launch plan holds its address, so its allocation must not make TrainStep drop them"""
    key = (device.index, stream())
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        release(ws, "workspace:" + tag)
        ws = cache[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)
    return ws


def seg_log_panel_tags(n):
    return ["Image/%d" % i for i in range(n)]


def seg_log_panels(inputs, logits, n=10, out=None):
    """the pictures of the segmentation trainer's log event (reference preprocessing/segmentation/logger.py:28-42) for the first
    min(n, B) samples, in two launches on the current stream: inputs = the batch ('image' float32 [B, 3, H, W], 'ground_mask' float32
    [B, H, W]); logits = the full-resolution logit map float32 [B, 1, H, W] or [B, H, W], dense or a `[:, 0:1]` view of the engine's
    [B, 2, H, W] head buffer (its batch stride is passed through, nothing is copied; any other non-contiguity raises)
    -> (uint8 device tensor [n, H, 3 W, 3]: image | ground truth | prediction, the tags "Image/0", ...)"""
    lib = _lib.load()
    image, mask = inputs["image"], inputs["ground_mask"]
    if image.dim() != 4 or image.shape[1] != 3 or not image.is_cuda:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: image must be a float32 CUDA tensor [B, 3, H, W]")
    B, _, H, W = image.shape
    if logits.dim() == 3:
        logits = logits.unsqueeze(1)
    if tuple(logits.shape) != (B, 1, H, W) or logits.dtype != torch.float32 or logits.device != image.device:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: logits must be float32 [B, 1, H, W] beside the image")
    if mask.numel() != B * H * W:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: ground_mask must be [B, H, W]")
    sb, _, sh, sw = logits.stride()
    if B == 1:
        sb = H * W
    if (W > 1 and sw != 1) or (H > 1 and sh != W) or sb < H * W:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: logits must be dense planes at a batch stride >= H * W "
                           "(a [:, 0:1] view of a contiguous [B, C, H, W] buffer), got strides %r" % (tuple(logits.stride()),))
    n = min(int(n), B)
    if out is None:
        out = torch.empty((n, H, 3 * W, 3), dtype=torch.uint8, device=image.device)
    if out.dtype != torch.uint8 or out.numel() != n * H * W * 9:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: out must be uint8 [%d, %d, %d, 3]" % (n, H, 3 * W))
    need = lib.fp_seg_log_panels_workspace(n, H, W)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.seg_log_panels: bad sizes, or too large")
    ws = _own_workspace(_stretch_workspaces, "seg_log_panels", need, image.device)
    _lib.check(lib.fp_seg_log_panels(_f32(image, "image"), _f32(mask, "ground_mask"), logits.data_ptr(), int(sb),
                                     _chk(_colour_lut("plasma", "float32", image.device)), _chk(out, "out"), B, n, H, W, ws.data_ptr(), ws.numel(),
                                     stream()), "fp_seg_log_panels")
    return out.view(n, H, 3 * W, 3), seg_log_panel_tags(n)


def stretch_colour(maps, cmap="viridis", out=None):
    """matplotlib's `plt.imsave` of 2-D arrays (Normalize by the map's own minimum and maximum, the colour map with bytes=True), in two
    launches on the current stream: maps = a CUDA tensor [B, H, W] or [H, W] of float32, uint8 or bool, finite
    -> uint8 device tensor [B, H, W, 3] (or [H, W, 3])"""
    lib = _lib.load()
    if not maps.is_cuda or maps.dim() not in (2, 3) or maps.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise RuntimeError("footprints_amd.ops.stretch_colour: maps must be a CUDA tensor [B, H, W] or [H, W] of float32, uint8 or bool")
    single = maps.dim() == 2
    m = maps.unsqueeze(0) if single else maps
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if not m.is_contiguous():
        m = m.contiguous()
    B, H, W = m.shape
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=m.device)
    if out.dtype != torch.uint8 or out.numel() != B * H * W * 3:
        raise RuntimeError("footprints_amd.ops.stretch_colour: out must be uint8 [%d, %d, %d, 3]" % (B, H, W))
    need = lib.fp_stretch_colour_workspace(B, H, W)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.stretch_colour: bad sizes, or too large")
    ws = workspace(need, m.device, "stretch")
    _lib.check(lib.fp_stretch_colour(_chk(m, "maps"), 1 if m.dtype == torch.uint8 else 0, _chk(_colour_lut(cmap, "bytes", m.device)),
                                     _chk(out, "out"), B, H, W, ws.data_ptr(), ws.numel(), stream()), "fp_stretch_colour")
    return out.view(H, W, 3) if single else out.view(B, H, W, 3)


# ---- output stage of the ground-segmentation network's inference mode (csrc/seg_infer.hip) ---------------------------------------------------
def seg_pack(logits, image=None, want_f32=False, want_picture=False, out=None):
    """sigmoid + float16 rounding (+ the reference's test picture) of full-resolution logits in one launch: logits float32 [B, 1, H, W],
    dense or a `[:, 0:1]` view of the engine's [B, 2, H, W] head buffer (its batch stride is passed through, nothing is copied; any other
    non-contiguity raises); image float32 [B, 3, H, W] in [0, 1], needed for the picture.  out = (half, f32, picture): buffers to write
    into, each None or a contiguous tensor of the right shape and type.
    -> (float16 [B, 1, H, W], float32 [B, 1, H, W] or None, uint8 [B, H, 2 W, 3] or None): the .npy contents of the reference's
    save_result, the sigmoid before the rounding, matplotlib's imsave of [image | plasma(prediction)] byte for byte"""
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise RuntimeError("footprints_amd.ops.seg_pack: logits must be a float32 CUDA tensor [B, 1, H, W]")
    B, _, H, W = logits.shape
    if min(B, H, W) < 1:
        raise RuntimeError("footprints_amd.ops.seg_pack: empty logits")
    sb, _, sh, sw = logits.stride()
    if B == 1:
        sb = H * W
    if (W > 1 and sw != 1) or (H > 1 and sh != W) or sb < H * W:
        raise RuntimeError("footprints_amd.ops.seg_pack: logits must be dense planes at a batch stride >= H * W "
                           "(a [:, 0:1] view of a contiguous [B, C, H, W] buffer), got strides %r" % (tuple(logits.stride()),))
    half, f32, picture = out if out is not None else (None, None, None)
    dev = logits.device
    if half is None:
        half = torch.empty((B, 1, H, W), dtype=torch.float16, device=dev)
    if want_f32 and f32 is None:
        f32 = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    if want_picture and picture is None:
        picture = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device=dev)
    if not want_f32:
        f32 = None
    if not want_picture:
        picture = None
    if half.dtype != torch.float16 or half.numel() != B * H * W or (f32 is not None and (f32.dtype != torch.float32 or f32.numel() != B * H * W)) \
            or (picture is not None and (picture.dtype != torch.uint8 or picture.numel() != B * H * W * 6)):
        raise RuntimeError("footprints_amd.ops.seg_pack: out buffers must be float16 / float32 [B, 1, H, W] and uint8 [B, H, 2 W, 3]")
    if want_picture and (image is None or tuple(image.shape) != (B, 3, H, W)):
        raise RuntimeError("footprints_amd.ops.seg_pack: the picture needs image float32 [B, 3, H, W]")
    _lib.check(_lib.load().fp_seg_pack(logits.data_ptr(), int(sb), _f32(image, "image") if want_picture else None, _chk(half, "half"),
                                       _f32(f32, "f32") if f32 is not None else None, _chk(picture, "picture") if picture is not None else None,
                                       _chk(_vis_lut(dev)) if want_picture else None, B, H, W, stream()), "fp_seg_pack")
    return half, f32, picture


# ---- output stage of the main network's test-set inference (csrc/infer_pack.hip) -------------------------------------------------------------
def infer_pack(pred, image=None, want_picture=False, out=None):
    """pack_pred_fp16 and vis_side_by_side in one launch over the logits: pred float32 [B, 4, H, W]; image float32 [B, 3, H, W] in
    [0, 1], needed for the picture.  out = (half, picture): buffers to write into, each None or a contiguous tensor of the right shape
    and type (a `[:n]` slice of a slot's buffer).
    -> (float16 [B, 4, H, W], bit-equal to pack_pred_fp16; uint8 [B, H, 2 W, 3], byte-equal to vis_side_by_side, or None)"""
    if pred.dim() != 4 or pred.shape[1] != 4 or not pred.is_cuda:
        raise RuntimeError("footprints_amd.ops.infer_pack: pred must be the 4-channel network output [B, 4, H, W] on the device")
    B, _, H, W = pred.shape
    if min(B, H, W) < 1:
        raise RuntimeError("footprints_amd.ops.infer_pack: empty prediction")
    half, picture = out if out is not None else (None, None)
    if half is None:
        half = torch.empty((B, 4, H, W), dtype=torch.float16, device=pred.device)
    if want_picture and picture is None:
        picture = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device=pred.device)
    if not want_picture:
        picture = None
    if half.dtype != torch.float16 or half.numel() != B * 4 * H * W or \
            (picture is not None and (picture.dtype != torch.uint8 or picture.numel() != B * H * W * 6)):
        raise RuntimeError("footprints_amd.ops.infer_pack: out buffers must be float16 [B, 4, H, W] and uint8 [B, H, 2 W, 3]")
    if want_picture and (image is None or tuple(image.shape) != (B, 3, H, W)):
        raise RuntimeError("footprints_amd.ops.infer_pack: the picture needs image float32 [B, 3, H, W]")
    colours = _vis_luts.get("side_by_side")                 # the table's first and last colour as r | g << 8 | b << 16
    if colours is None:
        lut = vis_colour_table()
        colours = _vis_luts["side_by_side"] = tuple(int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16 for c in (lut[0], lut[255]))
    _lib.check(_lib.load().fp_infer_pack(_f32(pred, "pred"), _f32(image, "image") if want_picture else None, _chk(half, "half"),
                                         _chk(picture, "picture") if picture is not None else None, colours[0], colours[1],
                                         B, H, W, stream()), "fp_infer_pack")
    return half, picture


# ---- baseline JPEG encoder (csrc/jpeg.hip) -------------------------------------------------------------------------------------------------
class JpegTables:
    """what a file of the installed Pillow at one quality is made of, parsed from the bytes up to and including the SOS segment:
    header (those bytes), size_at (index of SOF0's two big-endian height bytes, the width's follow), quant {table id: 64 values in zigzag
    order}, huff {class << 4 | id: {symbol: (code, length)}}, words (uint32 numpy: the code table of fp_jpeg_encode)"""

    def __init__(self, data):
        import numpy as np
        self.quant, self.huff, self.size_at = {}, {}, None
        if data[:2] != b"\xff\xd8":
            raise ValueError("not a JPEG file")
        i = 2
        while True:
            if data[i] != 0xFF:
                raise ValueError("JPEG header: marker expected at byte %d" % i)
            marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
            body = data[i + 4:i + 2 + length]
            if marker == 0xDB:                                      # DQT: 8-bit tables, zigzag order
                for p in range(0, len(body), 65):
                    if body[p] >> 4:
                        raise ValueError("JPEG header: 16-bit quantisation table")
                    self.quant[body[p] & 15] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8).astype(np.int64)
            elif marker == 0xC4:                                    # DHT: canonical codes from the 16 counts and the values
                p = 0
                while p < len(body):
                    counts = body[p + 1:p + 17]
                    values = body[p + 17:p + 17 + sum(counts)]
                    code, k, table = 0, 0, {}
                    for length_bits in range(1, 17):
                        for _ in range(counts[length_bits - 1]):
                            table[values[k]] = (code, length_bits)
                            code += 1
                            k += 1
                        code <<= 1
                    self.huff[body[p]] = table
                    p += 17 + len(values)
            elif marker == 0xC0:                                    # SOF0: precision, height, width, components
                if body[0] != 8 or body[5] != 3 or bytes(body[6:15]) != b"\x01\x22\x00\x02\x11\x01\x03\x11\x01":
                    raise ValueError("JPEG header: not 8-bit YCbCr 4:2:0 with tables 0, 1, 1")
                self.size_at = i + 5
            elif marker in (0xC1, 0xC2, 0xC9, 0xCA, 0xDD):
                raise ValueError("JPEG header: not a baseline file without restart markers")
            elif marker == 0xDA:
                self.header = bytes(data[:i + 2 + length])
                break
            i += 2 + length
        if self.size_at is None or sorted(self.quant) != [0, 1] or sorted(self.huff) != [0x00, 0x01, 0x10, 0x11]:
            raise ValueError("JPEG header: two quantisation and four Huffman tables expected")
        words = np.zeros(_lib.JPEG_TABLE_WORDS, dtype=np.uint32)
        for t in (0, 1):
            words[64 * t:64 * t + 64] = self.quant[t]
            for sym, (code, n) in self.huff[t].items():
                words[128 + 16 * t + sym] = code | n << 16
            for sym, (code, n) in self.huff[0x10 | t].items():
                words[160 + 256 * t + sym] = code | n << 16
        self.words = words
        self._device = {}

    def file_header(self, h, w):
        """the header of an h x w picture: the parsed bytes with SOF0's size patched"""
        at = self.size_at
        return self.header[:at] + bytes((h >> 8, h & 255, w >> 8, w & 255)) + self.header[at + 4:]

    def device_words(self, device):
        t = self._device.get(device)
        if t is None:
            t = self._device[device] = torch.from_numpy(self.words.view("int32").copy()).to(device)
        return t


_jpeg_tables = {}


def jpeg_tables(quality=95, dpi=None):
    """JpegTables of the installed Pillow at `quality`: a small RGB dummy is encoded once per (quality, dpi) and its header parsed; nothing
    of a JPEG header is compiled into this package.  dpi = None, or the (x, y) pair handed to Pillow's save: it changes the JFIF unit and
    density bytes of the header and nothing else (matplotlib's imsave writes dpi=(100, 100))"""
    key = (int(quality), None if dpi is None else (dpi[0], dpi[1]))
    t = _jpeg_tables.get(key)
    if t is None:
        import io
        import numpy as np
        from PIL import Image
        buf = io.BytesIO()
        extra = {} if dpi is None else {"dpi": key[1]}
        Image.fromarray(np.zeros((16, 16, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=int(quality), **extra)
        t = _jpeg_tables[key] = JpegTables(buf.getvalue())
    return t


def jpeg_records(shapes):
    """fp_jpeg_sample records of pictures of `shapes` = [(h, w), ...] lying one after the other in a packed buffer
    -> (records uint8 numpy, bytes of the packed buffer, max_h, max_w)"""
    import numpy as np
    rec = (_lib.JpegSample * len(shapes))()
    off = 0
    for b, (h, w) in enumerate(shapes):
        rec[b] = _lib.JpegSample(off, h, w)
        off += h * w * 3
    return np.frombuffer(bytes(rec), dtype=np.uint8).copy(), off, max(s[0] for s in shapes), max(s[1] for s in shapes)


def jpeg_max_scan_bytes(B, max_h, max_w):
    """the largest output jpeg_encode_packed can need for B pictures of at most max_h x max_w"""
    n = _lib.load().fp_jpeg_max_scan_bytes(B, max_h, max_w)
    if n < 0:
        raise RuntimeError("footprints_amd.ops.jpeg_max_scan_bytes: bad sizes, or too large")
    return n


def jpeg_encode_packed(src, src_bytes, samples, B, quality=95, out=None, max_h=None, max_w=None, table=None):
    """device half of the encoder: `src` the packed pictures (uint8 device buffer, src_bytes used), `samples` B fp_jpeg_sample records on
    the device (jpeg_records), max_h / max_w the largest height and width among them (required: the records are not read here)
    -> (out, table): `out` uint8 device buffer holding the entropy-coded scans back to back (default: one of the worst-case size; a given
    one may be smaller), `table` int64 device [B + 1, 2]: offset and length of each scan, last row = bytes written, status (1: a record
    was turned down or a scan did not fit; that sample has length 0 and nothing of it was written).  Does not wait for the device."""
    lib = _lib.load()
    if max_h is None or max_w is None:
        raise ValueError("footprints_amd.ops.jpeg_encode_packed: max_h and max_w are required")
    need = lib.fp_jpeg_workspace_bytes(B, max_h, max_w)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.jpeg_encode_packed: bad sizes, or too large")
    if src.dtype != torch.uint8 or src.numel() < src_bytes:
        raise RuntimeError("footprints_amd.ops.jpeg_encode_packed: src must be a uint8 buffer of at least src_bytes bytes")
    if samples.numel() * samples.element_size() < B * C.sizeof(_lib.JpegSample):
        raise RuntimeError("footprints_amd.ops.jpeg_encode_packed: fewer than B sample records")
    if out is None:
        out = torch.empty(jpeg_max_scan_bytes(B, max_h, max_w), dtype=torch.uint8, device=src.device)
    if table is None:
        table = torch.empty((B + 1, 2), dtype=torch.int64, device=src.device)
    if out.dtype != torch.uint8 or table.dtype != torch.int64 or table.numel() < 2 * (B + 1):
        raise RuntimeError("footprints_amd.ops.jpeg_encode_packed: out must be uint8 and table int64 [B + 1, 2]")
    ws = workspace(need, src.device, "jpeg")
    words = jpeg_tables(quality).device_words(src.device)
    _lib.check(lib.fp_jpeg_encode(_chk(src, "src"), int(src_bytes), _chk(samples, "samples"), _chk(words), _chk(out, "out"), out.numel(),
                                  _chk(table, "table"), B, max_h, max_w, ws.data_ptr(), ws.numel(), stream()), "fp_jpeg_encode")
    return out, table


def jpeg_files(scans, table, shapes, quality=95, dpi=None):
    """complete files from the encoder's output on the HOST: scans (bytes-like, at least the bytes the table's last row counts), table
    (int64 [B + 1, 2] numpy), shapes [(h, w), ...] -> list of bytes: header + scan + EOI"""
    if int(table[len(shapes)][1]) != 0:
        raise ValueError("footprints_amd.ops.jpeg_encode: a sample record was turned down on the device, or the output buffer was too small")
    t = jpeg_tables(quality, dpi)
    view = memoryview(scans)
    return [t.file_header(h, w) + bytes(view[int(table[b][0]):int(table[b][0]) + int(table[b][1])]) + b"\xff\xd9" for b, (h, w) in enumerate(shapes)]


def jpeg_encode(pictures, quality=95, dpi=None):
    """Pillow's `Image.fromarray(p).save(f, format="JPEG", quality=quality)` (with `dpi=dpi` when one is given: only the files' headers
    differ) for a batch, byte for byte (Pillow on libjpeg-turbo), encoded on the device: pictures = a uint8 device tensor [B, H, W, 3], or a list of numpy uint8 [h, w, 3] of any sizes (uploaded here)
    -> list of B bytes objects, each a complete file.  Copies the length table, waits, copies exactly the bytes used."""
    import numpy as np
    if torch.is_tensor(pictures):
        if pictures.dim() != 4 or pictures.shape[3] != 3 or pictures.dtype != torch.uint8 or not pictures.is_cuda:
            raise ValueError("footprints_amd.ops.jpeg_encode: a tensor of pictures must be uint8 [B, H, W, 3] on the device")
        shapes = [(int(pictures.shape[1]), int(pictures.shape[2]))] * int(pictures.shape[0])
        packed = pictures.contiguous().view(-1)
    else:
        if any(p.dtype != np.uint8 or p.ndim != 3 or p.shape[2] != 3 for p in pictures):
            raise ValueError("footprints_amd.ops.jpeg_encode: pictures must be uint8 [h, w, 3]")
        shapes = [(int(p.shape[0]), int(p.shape[1])) for p in pictures]
        packed = torch.from_numpy(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pictures])).cuda()
    if not shapes:
        return []
    records, total, max_h, max_w = jpeg_records(shapes)
    out, table = jpeg_encode_packed(packed, total, torch.from_numpy(records).to(packed.device), len(shapes), quality, max_h=max_h, max_w=max_w)
    table = table.cpu().numpy()                  # waits
    used = int(table[len(shapes)][0])
    return jpeg_files(out[:used].cpu().numpy().tobytes() if used else b"", table, shapes, quality, dpi)


# ---- baseline JPEG decoder (csrc/jpeg_decode.hip) ------------------------------------------------------------------------------------------
# Both defaults rest on the bench batch of profiles/jpeg_decode_notes.md (12 picture-like 375 x 1242 frames, quality 95, 4:2:0): 256 and
# 512 bits were the fastest lengths, 512 by 1 to 2 %, and 256 keeps noise at quality 100 on the fallback path (the notes say why that
# decided); the launch budget is twice the most launches a file of the batch needed to settle.
JPEG_DECODE_SUBSEQ_BITS = 256
JPEG_DECODE_MAX_ROUNDS = 4
_JPEG_NATURAL = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class _JpegHost(Exception):
    """the reason a file is decoded on the host"""


def _jpeg_parse(data):
    import numpy as np
    n_data = len(data)
    if n_data < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise _JpegHost("no start-of-image marker")
    quant, huff, frame, jfif, i = {}, {}, None, False, 2
    while True:
        if i + 4 > n_data:
            raise _JpegHost("the header is cut")
        if data[i] != 0xFF:
            raise _JpegHost("marker expected at byte %d" % i)
        marker = data[i + 1]
        if marker == 0xFF:                                          # fill byte
            i += 1
            continue
        length = (data[i + 2] << 8) | data[i + 3]
        if length < 2 or i + 2 + length > n_data:
            raise _JpegHost("segment length %d at byte %d" % (length, i))
        body = bytes(data[i + 4:i + 2 + length])
        if marker == 0xE0:
            jfif = jfif or (length >= 16 and body[:5] == b"JFIF\0")
        elif marker == 0xEE:
            if body[:5] == b"Adobe":
                raise _JpegHost("Adobe marker")
        elif marker == 0xDB:
            p = 0
            while p < len(body):
                if body[p] >> 4 or (body[p] & 15) > 3 or p + 65 > len(body):
                    raise _JpegHost("quantisation table of 16 bits, or cut")
                quant[body[p] & 15] = body[p + 1:p + 65]            # zigzag order
                p += 65
        elif marker == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body) or (body[p] >> 4) > 1 or (body[p] & 15) > 1:
                    raise _JpegHost("Huffman table id")
                counts = body[p + 1:p + 17]
                total = sum(counts)
                values = body[p + 17:p + 17 + total]
                if total > 256 or len(values) != total:
                    raise _JpegHost("Huffman table cut")
                code = 0
                for bits in range(1, 17):                           # the codes of a length must fit into it
                    code += counts[bits - 1]
                    if code > (1 << bits):
                        raise _JpegHost("Huffman table over-subscribed")
                    code <<= 1
                if (body[p] >> 4) == 0 and any(v > 15 for v in values):
                    raise _JpegHost("DC category above 15")
                huff[(body[p] >> 4, body[p] & 15)] = (counts, values)
                p += 17 + total
        elif marker == 0xC0:
            if frame is not None or len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise _JpegHost("frame header")
            if body[0] != 8:
                raise _JpegHost("%d-bit samples" % body[0])
            frame = ((body[1] << 8) | body[2], (body[3] << 8) | body[4],
                     [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])])
        elif 0xC1 <= marker <= 0xCF:                                # C4 was taken above
            raise _JpegHost("not baseline sequential Huffman (SOF%d)" % (marker - 0xC0))
        elif marker == 0xDD:
            if len(body) == 2 and (body[0] or body[1]):
                raise _JpegHost("restart interval")
        elif marker == 0xDA:
            break
        elif marker in (0x01, 0xD8, 0xD9, 0xDC) or 0xD0 <= marker <= 0xD7:
            raise _JpegHost("marker %02X in the header" % marker)
        i += 2 + length
    if frame is None:
        raise _JpegHost("scan before the frame header")
    h, w, comps = frame
    if h < 1 or w < 1:
        raise _JpegHost("empty picture")
    if len(comps) not in (1, 3):
        raise _JpegHost("%d components" % len(comps))
    if len(body) != 4 + 2 * len(comps) or body[0] != len(comps):
        raise _JpegHost("not one scan of all components")
    if body[1 + 2 * len(comps):] != b"\x00\x3f\x00":
        raise _JpegHost("spectral selection or successive approximation")
    tq, td, ta = [], [], []
    for c, (ident, _, _, q) in enumerate(comps):
        if body[1 + 2 * c] != ident:
            raise _JpegHost("scan components out of order")
        tq.append(q)
        td.append(body[2 + 2 * c] >> 4)
        ta.append(body[2 + 2 * c] & 15)
        if q not in quant or (0, td[-1]) not in huff or (1, ta[-1]) not in huff:
            raise _JpegHost("a table the file does not define")
    if len(comps) == 1:
        if comps[0][1:3] != (1, 1):
            raise _JpegHost("grey with sampling factors")
        hs = vs = 1
    else:
        if not jfif and [c[0] for c in comps] != [1, 2, 3]:
            raise _JpegHost("not YCbCr by libjpeg's rule")
        hs, vs = comps[0][1:3]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
            raise _JpegHost("sampling %r" % ([c[1:3] for c in comps],))
    start = i + 2 + length
    a = np.frombuffer(data, dtype=np.uint8)[start:]
    marks = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0)) if a.size > 1 else np.zeros(0, np.int64)
    if marks.size == 0 or marks[0] == 0:
        raise _JpegHost("no entropy-coded segment, or no marker behind it")
    if a[marks[0] + 1] != 0xD9:
        raise _JpegHost("marker %02X inside the scan (restart markers, or several scans)" % a[marks[0] + 1])
    if int(marks[0]) >= 1 << 28:
        raise _JpegHost("scan of 256 MiB or more")
    return dict(h=h, w=w, ncomp=len(comps), hs=hs, vs=vs, tq=tuple(tq), td=tuple(td), ta=tuple(ta), quant=quant, huff=huff,
                scan_offset=start, scan_bytes=int(marks[0]))


def jpeg_parse(data):
    """the markers of a JPEG file (bytes) -> a dict: device=True with h, w, ncomp, hs, vs (luma sampling), tq / td / ta (per component
    the quantisation, DC and AC table ids), quant {id: 64 bytes in zigzag order}, huff {(class, id): (16 counts, symbols)}, scan_offset
    and scan_bytes of the entropy-coded segment -- or device=False with the reason the file goes to Pillow.  Accepted: SOF0, 8 bits, one
    interleaved scan, no restart interval, no Adobe marker, grey or YCbCr (JFIF marker, or component ids 1, 2, 3) with chroma 1x1 and
    luma 1x1, 2x1 or 2x2.  Never raises on a damaged header."""
    try:
        info = _jpeg_parse(data if isinstance(data, (bytes, bytearray)) else bytes(data))
    except (_JpegHost, IndexError) as e:
        return dict(device=False, reason=str(e) or "the header is cut")
    info["device"] = True
    return info


def _jpeg_huff_words(counts, values):
    """one Huffman table of a table block (fp_jpeg_decode_table_words in include/footprints_hip.h)"""
    import numpy as np
    words = np.zeros(356, dtype=np.int64)
    packed = np.zeros(256, dtype=np.int64)
    packed[:len(values)] = list(values)
    code, k = 0, 0
    for bits in range(1, 17):
        n = counts[bits - 1]
        words[274 + bits] = k - code                                # valptr - mincode
        for _ in range(n):
            if bits <= 8:
                words[code << (8 - bits):(code + 1) << (8 - bits)] = bits << 8 | values[k]
            code += 1
            k += 1
        words[256 + bits] = code - 1 if n else -1                   # maxcode
        code <<= 1
    words[256] = words[273] = -1
    words[292:356] = packed[0::4] | packed[1::4] << 8 | packed[2::4] << 16 | packed[3::4] << 24
    return words


def _jpeg_table_block(info):
    import numpy as np
    words = np.zeros(_lib.JPEG_DECODE_TABLE_WORDS, dtype=np.int64)
    for c in range(info["ncomp"]):
        words[4 * c:4 * c + 3] = (info["tq"][c], info["td"][c], info["ta"][c])
    for t, q in info["quant"].items():
        nat = np.zeros(64, dtype=np.int64)
        nat[list(_JPEG_NATURAL)] = list(q)
        words[16 + 64 * t:16 + 64 * t + 64] = nat
    for (cls, t), (counts, values) in info["huff"].items():
        at = 272 + 356 * (2 * cls + t)
        words[at:at + 356] = _jpeg_huff_words(counts, values)
    return (words & 0xFFFFFFFF).astype(np.uint32)


_jpeg_table_blocks = {}


def jpeg_decode_pack(files, infos=None, out_offsets=None, pinned=False, rects=None):
    """host half of the decoder for files jpeg_parse accepted: their entropy-coded segments one after the other in one uint8 buffer
    (pinned=True: a pinned torch tensor's), the fp_jpeg_decode_sample records, and one table block per distinct set of tables and
    selectors (most files share the standard tables).  out_offsets: where each picture goes in the output (default: one after the other)
    -> dict(scans, scan_bytes, records, tables, n_sets, B, shapes, out_bytes, max_h, max_w, max_scan).
    rects: one (y0, x0, rh, rw) per file -- the pack is then jpeg_decode_window_packed's: fp_jpeg_decode_window_sample records, the output
    holds the windows (dense [rh][rw][3]), and the dict also has rects, max_win_h and max_win_w.  A rectangle is not checked here: the device
    refuses, per sample, one that is empty or not inside its picture."""
    import numpy as np
    infos = [jpeg_parse(f) for f in files] if infos is None else infos
    if not files or any(not i["device"] for i in infos):
        raise ValueError("footprints_amd.ops.jpeg_decode_pack: needs at least one file, and only files jpeg_parse accepts")
    if rects is not None and len(rects) != len(files):
        raise ValueError("footprints_amd.ops.jpeg_decode_pack: one rectangle per file")
    total = sum(i["scan_bytes"] for i in infos)
    holder = torch.empty(total, dtype=torch.uint8).pin_memory() if pinned else None
    scans = holder.numpy() if pinned else np.empty(total, dtype=np.uint8)
    rec = ((_lib.JpegDecodeSample if rects is None else _lib.JpegDecodeWindowSample) * len(files))()
    sets, blocks, at, out_at = {}, [], 0, 0
    for b, (f, i) in enumerate(zip(files, infos)):
        key = (i["tq"], i["td"], i["ta"], tuple(sorted(i["quant"].items())), tuple(sorted(i["huff"].items())))
        block = _jpeg_table_blocks.get(key)
        if block is None:
            if len(_jpeg_table_blocks) > 256:
                _jpeg_table_blocks.clear()
            block = _jpeg_table_blocks[key] = _jpeg_table_block(i)
        if key not in sets:
            sets[key] = len(blocks)
            blocks.append(block)
        scans[at:at + i["scan_bytes"]] = np.frombuffer(f, dtype=np.uint8, count=i["scan_bytes"], offset=i["scan_offset"])
        off = out_at if out_offsets is None else int(out_offsets[b])
        fields = (at, off, i["scan_bytes"], i["h"], i["w"], i["ncomp"], i["hs"], i["vs"], sets[key], 0)
        if rects is None:
            rec[b] = _lib.JpegDecodeSample(*fields)
            out_at += i["h"] * i["w"] * 3
        else:
            y0, x0, rh, rw = (int(v) for v in rects[b])
            rec[b] = _lib.JpegDecodeWindowSample(*fields, y0, x0, rh, rw)
            out_at += max(rh, 0) * max(rw, 0) * 3
        at += i["scan_bytes"]
    pack = dict(scans=holder if pinned else scans, scan_bytes=total, records=np.frombuffer(bytes(rec), dtype=np.uint8).copy(),
                tables=np.concatenate(blocks), n_sets=len(blocks), B=len(files), shapes=[(i["h"], i["w"]) for i in infos], out_bytes=out_at,
                max_h=max(i["h"] for i in infos), max_w=max(i["w"] for i in infos), max_scan=max(i["scan_bytes"] for i in infos))
    if rects is not None:
        pack.update(jpeg_window_bounds(rects, pack["max_h"], pack["max_w"]), rects=[tuple(int(v) for v in r) for r in rects])
    return pack


def jpeg_window_bounds(rects, max_h, max_w):
    """max_win_h / max_win_w of a call: the largest rectangle, kept inside 1..max_h / 1..max_w (a rectangle beyond is refused on the device)"""
    return dict(max_win_h=min(max(1, max(int(r[2]) for r in rects)), max_h), max_win_w=min(max(1, max(int(r[3]) for r in rects)), max_w))


def jpeg_decode_packed(pack, out=None, out_bytes=None, subseq_bits=None, max_rounds=None, status=None, device="cuda", want_info=False):
    """device half: uploads the scans, records and table blocks of `pack` (jpeg_decode_pack) and decodes into `out` (uint8 device buffer,
    default: one of pack["out_bytes"]; out_bytes: how much of it may be written), the packed layout resize_u8_packed, vis_overlay_device
    and jpeg_encode_packed read -> (out, shapes, status): status int32 device [B + 1], per sample and their maximum: 0 decoded, 1 record
    turned down, 2 not settled within max_rounds launches, 3 corrupt stream; a sample with a non-zero status wrote nothing.  Does not
    wait for the device.  want_info=True appends the kernels' counters, int32 device [B, 8] (include/footprints_hip.h)."""
    if "rects" in pack:
        raise ValueError("footprints_amd.ops.jpeg_decode_packed: the pack holds rectangles (jpeg_decode_window_packed)")
    return _jpeg_decode_launch(pack, out, out_bytes, subseq_bits, max_rounds, status, device, want_info)


def jpeg_decode_window_packed(pack, rects=None, out=None, out_offsets=None, out_bytes=None, subseq_bits=None, max_rounds=None, status=None,
                              device="cuda", want_info=False):
    """jpeg_decode_packed for one rectangle (y0, x0, rh, rw) per file (fp_jpeg_decode_window): `out` receives the bytes the whole picture
    has at [y0:y0+rh, x0:x0+rw], dense [rh][rw][3] at the sample's offset, and nothing else -> (out, windows [(rh, rw)], status).  pack:
    jpeg_decode_pack(files, rects=...) -- every array may be pinned, nothing is rebuilt -- or a plain pack with `rects` (and out_offsets,
    default: one window after the other) given here, from which the window records are written.  A rectangle that is empty or not inside
    its picture gives that sample status 1; the others are unaffected.  Does not wait for the device."""
    if rects is not None:
        import numpy as np
        if "rects" in pack or len(rects) != pack["B"] or (out_offsets is not None and len(out_offsets) != pack["B"]):
            raise ValueError("footprints_amd.ops.jpeg_decode_window_packed: one rectangle (and offset) per file, for a pack without rectangles")
        plain = (_lib.JpegDecodeSample * pack["B"]).from_buffer_copy(np.asarray(pack["records"]).tobytes())
        rec = (_lib.JpegDecodeWindowSample * pack["B"])()
        at = 0
        for b, r in enumerate(rects):
            y0, x0, rh, rw = (int(v) for v in r)
            p = plain[b]
            rec[b] = _lib.JpegDecodeWindowSample(p.scan_offset, at if out_offsets is None else int(out_offsets[b]), p.scan_bytes, p.h, p.w, p.ncomp,
                                                 p.hs, p.vs, p.table_set, 0, y0, x0, rh, rw)
            at += max(rh, 0) * max(rw, 0) * 3
        pack = dict(pack, records=np.frombuffer(bytes(rec), dtype=np.uint8).copy(), rects=[tuple(int(v) for v in r) for r in rects],
                    out_bytes=at if out_offsets is None else max(int(o) + max(int(r[2]), 0) * max(int(r[3]), 0) * 3 for o, r in zip(out_offsets, rects)),
                    tables=np.asarray(pack["tables"]), **jpeg_window_bounds(rects, pack["max_h"], pack["max_w"]))
    elif "rects" not in pack:
        raise ValueError("footprints_amd.ops.jpeg_decode_window_packed: no rectangles, neither in the pack nor in the call")
    got = _jpeg_decode_launch(pack, out, out_bytes, subseq_bits, max_rounds, status, device, want_info)
    return (got[0], [(r[2], r[3]) for r in pack["rects"]]) + tuple(got[2:])


def _jpeg_decode_launch(pack, out, out_bytes, subseq_bits, max_rounds, status, device, want_info):
    """jpeg_decode_packed and jpeg_decode_window_packed behind their checks: a pack with 'rects' goes to fp_jpeg_decode_window"""
    lib = _lib.load()
    B = pack["B"]
    subseq_bits = JPEG_DECODE_SUBSEQ_BITS if subseq_bits is None else int(subseq_bits)
    max_rounds = JPEG_DECODE_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    scans = pack["scans"] if torch.is_tensor(pack["scans"]) else torch.from_numpy(pack["scans"])
    d_scans = scans.to(device, non_blocking=True)
    if torch.is_tensor(pack["records"]):            # pinned by the caller (datasets/decode_stage.py): queued copies, no wait for the stream
        d_rec = pack["records"].to(device, non_blocking=True)
        d_tab = pack["tables"].to(device, non_blocking=True)
    else:
        d_rec = torch.from_numpy(pack["records"]).to(device)
        d_tab = torch.from_numpy(pack["tables"].view("int32")).to(device)
    if out is None:
        out = torch.empty(pack["out_bytes"], dtype=torch.uint8, device=d_scans.device)
    out_bytes = out.numel() if out_bytes is None else int(out_bytes)
    if status is None:
        status = torch.empty(B + 1, dtype=torch.int32, device=d_scans.device)
    if out.dtype != torch.uint8 or out.numel() < out_bytes or status.dtype != torch.int32 or status.numel() < B + 1:
        raise RuntimeError("footprints_amd.ops.jpeg_decode_packed: out must be uint8 of at least out_bytes and status int32 [B + 1]")
    need = lib.fp_jpeg_decode_workspace_bytes(B, pack["max_h"], pack["max_w"], pack["max_scan"], subseq_bits)
    if need < 0:
        raise RuntimeError("footprints_amd.ops.jpeg_decode_packed: bad sizes, or too large")
    ws = workspace(need, d_scans.device, "jpeg_decode")
    if "rects" in pack:
        _lib.check(lib.fp_jpeg_decode_window(_chk(d_scans, "scans"), int(pack["scan_bytes"]), _chk(d_rec, "samples"), _chk(d_tab, "tables"),
                                             pack["n_sets"], _chk(out, "out"), out_bytes, _chk(status, "status"), B, pack["max_h"], pack["max_w"],
                                             pack["max_win_h"], pack["max_win_w"], pack["max_scan"], subseq_bits, max_rounds, ws.data_ptr(),
                                             ws.numel(), stream()), "fp_jpeg_decode_window")
    else:
        _lib.check(lib.fp_jpeg_decode(_chk(d_scans, "scans"), int(pack["scan_bytes"]), _chk(d_rec, "samples"), _chk(d_tab, "tables"), pack["n_sets"],
                                      _chk(out, "out"), out_bytes, _chk(status, "status"), B, pack["max_h"], pack["max_w"], pack["max_scan"],
                                      subseq_bits, max_rounds, ws.data_ptr(), ws.numel(), stream()), "fp_jpeg_decode")
    if want_info:
        return out, pack["shapes"], status, ws[:B * 32].view(torch.int32).view(B, 8).clone()
    return out, pack["shapes"], status


def _jpeg_host_decode(data):
    import io
    import numpy as np
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def jpeg_decode(files, subseq_bits=None, max_rounds=None, return_status=False):
    """`np.asarray(PIL.Image.open(f).convert("RGB"))` of a list of files (bytes), byte for byte: the files jpeg_parse accepts are decoded
    on the device in one call, the others by Pillow on the host -- and so is a file the device turned down (status 1), did not settle
    within max_rounds (2) or found corrupt (3): then whatever Pillow returns or raises is the result.  WAITS for the device.
    return_status=True -> (arrays, statuses): the device's status per file, -1 for a file the parser sent to the host."""
    files = [bytes(f) for f in files]
    infos = [jpeg_parse(f) for f in files]
    on_device = [n for n, i in enumerate(infos) if i["device"]]
    arrays, statuses = [None] * len(files), [-1] * len(files)
    if on_device:
        pack = jpeg_decode_pack([files[n] for n in on_device], [infos[n] for n in on_device])
        out, shapes, status = jpeg_decode_packed(pack, subseq_bits=subseq_bits, max_rounds=max_rounds)
        status = status.cpu().numpy()               # waits
        host = out.cpu().numpy() if int(status[-1]) == 0 or (status[:-1] == 0).any() else None
        at = 0
        for j, n in enumerate(on_device):
            h, w = shapes[j]
            statuses[n] = int(status[j])
            if statuses[n] == 0:
                arrays[n] = host[at:at + h * w * 3].reshape(h, w, 3).copy()
            at += h * w * 3
    for n, f in enumerate(files):
        if arrays[n] is None:
            arrays[n] = _jpeg_host_decode(f)
    return (arrays, statuses) if return_status else arrays


def jpeg_decode_window(files, rects, subseq_bits=None, max_rounds=None, return_status=False):
    """`np.asarray(PIL.Image.open(f).convert("RGB"))[y0:y0+rh, x0:x0+rw]` for every file (bytes) and its rectangle (y0, x0, rh, rw), byte
    for byte: jpeg_decode's division of work, with the device decoding the rectangles alone.  A rectangle that is empty or not inside its
    picture is a ValueError.  WAITS for the device.  return_status=True -> (arrays, statuses) as jpeg_decode."""
    files = [bytes(f) for f in files]
    rects = [tuple(int(v) for v in r) for r in rects]
    if len(rects) != len(files):
        raise ValueError("footprints_amd.ops.jpeg_decode_window: one rectangle per file")

    def inside(n, h, w):
        y0, x0, rh, rw = rects[n]
        if rh < 1 or rw < 1 or y0 < 0 or x0 < 0 or y0 + rh > h or x0 + rw > w:
            raise ValueError("footprints_amd.ops.jpeg_decode_window: file %d: the rectangle %r is empty or not inside the picture of %d x %d"
                             % (n, rects[n], h, w))

    infos = [jpeg_parse(f) for f in files]
    on_device = [n for n, i in enumerate(infos) if i["device"]]
    for n in on_device:
        inside(n, infos[n]["h"], infos[n]["w"])
    arrays, statuses = [None] * len(files), [-1] * len(files)
    if on_device:
        pack = jpeg_decode_pack([files[n] for n in on_device], [infos[n] for n in on_device], rects=[rects[n] for n in on_device])
        out, windows, status = jpeg_decode_window_packed(pack, subseq_bits=subseq_bits, max_rounds=max_rounds)
        status = status.cpu().numpy()               # waits
        host = out.cpu().numpy() if (status[:-1] == 0).any() else None
        at = 0
        for j, n in enumerate(on_device):
            rh, rw = windows[j]
            statuses[n] = int(status[j])
            if statuses[n] == 0:
                arrays[n] = host[at:at + rh * rw * 3].reshape(rh, rw, 3).copy()
            at += rh * rw * 3
    for n, f in enumerate(files):
        if arrays[n] is None:
            frame = _jpeg_host_decode(f)
            inside(n, frame.shape[0], frame.shape[1])
            y0, x0, rh, rw = rects[n]
            arrays[n] = frame[y0:y0 + rh, x0:x0 + rw].copy()
    return (arrays, statuses) if return_status else arrays


def resize_records(shapes, H, W, tables, filter="lanczos"):
    """resize_pack's records for pictures of `shapes` = [(h, w), ...] (three channels) that lie one after the other in a packed buffer
    already -> (records uint8 numpy, bytes of the buffer, max_h, max_w)"""
    import numpy as np
    rec = (_lib.ResizeSample * len(shapes))()
    off = 0
    for b, (h, w) in enumerate(shapes):
        rec[b] = _lib.ResizeSample(off, h, w, tables.index(w, W, filter), tables.index(h, H, filter))
        off += h * w * 3
    return np.frombuffer(bytes(rec), dtype=np.uint8).copy(), off, max(s[0] for s in shapes), max(s[1] for s in shapes)
