"""The packed weight layouts of one convolution as ONE table: role x operand format (pure: host-side size queries only, no device).

A ROLE is what a launch multiplies by -- the whole filter (`fwd` / `dgrad`), the skip half of a conv over cat[nearest_x2(low C0), skip C1]
(`skip_*`: channels C0..C0+C1), or its upsampled half by output phase (`phase_*`: channels 0..C0).  A FORMAT is the operand arithmetic of
the kernel that reads the copy: `f32` (fp32 MFMA), `bf3` (exact three-term bf16 split), `hp` (scaled fp16 pairs, with the weight's amax slot).
`plan` lists the copies a convolution owns, in the order they lie in Engine.packed; `pack_jobs` orders them as a pack table does."""
from collections import namedtuple
from types import SimpleNamespace

from . import _lib as L
from . import ops

FORMATS = ("f32", "bf3", "hp")
Row = namedtuple("Row", "f32 bf3 hp")          # the L.PACK_* kind per format
TABLE = {                                       # role -> pack kinds; sizes: _numel, slices and ownership: plan
    "fwd": Row(L.PACK_FWD, L.PACK_FWD_BF3, L.PACK_FWD_HP),
    "dgrad": Row(L.PACK_DGRAD, L.PACK_DGRAD_BF3, L.PACK_DGRAD_HP),
    "skip_fwd": Row(L.PACK_FWD, L.PACK_FWD_BF3, L.PACK_FWD_HP),
    "skip_dgrad": Row(L.PACK_DGRAD, L.PACK_DGRAD_BF3, L.PACK_DGRAD_HP),
    "phase_fwd": Row(L.PACK_UP2_FWD, L.PACK_UP2_FWD_BF3, L.PACK_UP2_FWD_HP),
    "phase_dgrad": Row(L.PACK_UP2_DGRAD, L.PACK_UP2_DGRAD_BF3, L.PACK_UP2_DGRAD_HP),
}
ROLES = tuple(TABLE)
_F32_SUB = ("phase_fwd", "skip_fwd", "phase_dgrad", "skip_dgrad")
# where a copy lies in Engine.packed, per convolution ...
STORE_ORDER = [("fwd", "f32"), ("dgrad", "f32")] + [(r, "f32") for r in _F32_SUB] + [(r, f) for f in ("bf3", "hp") for r in ROLES]
# ... and where its job stands in a pack table (the fp16 pairs first: their amax pass runs over the same jobs)
JOB_ORDER = [("fwd", "f32"), ("dgrad", "f32")] + [(r, f) for f in ("hp", "bf3") for r in ROLES] + \
            [(r, "f32") for r in ("phase_fwd", "phase_dgrad", "skip_fwd", "skip_dgrad")]
STEM_HP_ELEMS = 11 * 64 * 16                    # FP_PACK_STEM_HP: 11 K-steps x 2 planes x 64 x 16 halves, in floats

Facts = namedtuple("Facts", "Cout Cin K stride stem head up2")          # up2 = (C0, C1) of a conv over cat[nearest_x2(low), skip], else None
Flags = namedtuple("Flags", "bf3 hp hp_igemm bf3_igemm phase hp_stem")  # the engine's format switches (engine.py: _BF3, _HP, ...)
# lazy: an fp32 copy that is packed on first use (Engine._need32); pooled: lies in Engine.packed (the stem's fp16-pair copy has its own buffer)
Layout = namedtuple("Layout", "role fmt kind numel c_begin c_count lazy pooled")


def classify(f, fl):
    """(bf3, hp, hp_ig, bf3_ig): split copies for the tile kernel (3x3 stride 1) / for the flattened kernel (3x3 stride 2, 1x1)"""
    bf3 = fl.bf3 and f.K == 3 and f.stride == 1 and not f.stem and not f.head
    flat = not bf3 and not f.stem and not f.head and f.K in (1, 3)
    return bf3, bf3 and fl.hp, fl.hp_igemm and flat, fl.bf3_igemm and flat and f.Cin % 4 == 0


def _numel(f, role, fmt, C0, C1):
    dg = role.endswith("dgrad")
    if role.startswith("phase"):
        n = ops.up2_packed_weight_elems(C0, f.Cout) if dg else ops.up2_packed_weight_elems(f.Cout, C0)
        return n * 3 // 2 if fmt == "bf3" else n            # three bf16 / two fp16 = one float per weight
    C = C1 if role.startswith("skip") else f.Cin
    if fmt == "f32":
        return ops.packed_weight_elems(f.Cout, C, f.K, dg, f.stem)
    return (ops.packed_weight_elems_bf3 if fmt == "bf3" else ops.packed_weight_elems_hp)(f.Cout, C, f.K, dg)


def plan(f, fl):
    """the layouts convolution `f` owns under the switches `fl`, in STORE_ORDER"""
    bf3, hp, hp_ig, bf3_ig = classify(f, fl)
    up2 = f.up2 if fl.phase else None
    C0, C1 = up2 if up2 else (0, 0)
    # an upsample conv launches by halves; of the whole filter it keeps the fp32 copies and, for small images, the forward concat pack
    whole = {"fwd": up2 is None or C1 != 0, "dgrad": up2 is None}
    split = {"f32": True, "bf3": bf3 or bf3_ig, "hp": hp or hp_ig or (f.stem and fl.hp and fl.hp_stem)}
    out = []
    for role, fmt in STORE_ORDER:
        if role.startswith("phase"):
            own, cb, cc = up2 is not None, 0, C0
        elif role.startswith("skip"):
            own, cb, cc = C1 != 0, C0, C1
        else:
            own, cb, cc = (whole[role] or fmt == "f32") and not (f.stem and role == "dgrad"), 0, f.Cin
        if not (own and split[fmt]):
            continue
        if f.stem:      # its own pack kinds: fp32 is read by every step (never lazy), the fp16-pair layout of the patch-in-LDS kernel has its own buffer
            out.append(Layout(role, fmt, L.PACK_STEM if fmt == "f32" else L.PACK_STEM_HP,
                              _numel(f, role, fmt, 0, 0) if fmt == "f32" else STEM_HP_ELEMS, cb, cc, False, fmt == "f32"))
        else:
            out.append(Layout(role, fmt, getattr(TABLE[role], fmt), _numel(f, role, fmt, C0, C1), cb, cc, fmt == "f32", True))
    return out


def pack_jobs(pairs, has_hp, hp_tile, two_term):
    """[(Layout, its tensor)] -> the ones a repack refreshes, in the order of a pack table.  A bf16 copy whose convolution also owns fp16
    pairs (has_hp) is packed only where a kernel still reads it: with the tile kernels on the exact split (not hp_tile), or -- tile
    layouts only -- for the two-term inference mode"""
    def live(l):
        return l.fmt != "bf3" or not has_hp or not hp_tile or (two_term and not l.role.startswith("phase"))
    return sorted((p for p in pairs if live(p[0])), key=lambda p: JOB_ORDER.index((p[0].role, p[0].fmt)))


class Formats:
    """the copies of one role: packed tensors (or None) per format + the amax slot the fp16 pairs were scaled by"""
    __slots__ = FORMATS + ("wslot",)

    def __init__(self, wslot=None):
        self.f32 = self.bf3 = self.hp = None
        self.wslot = wslot


def conv_layouts(wslot):
    """ConvRec.lay: one Formats per role (lay.dgrad.bf3, ...); all = [(Layout, its tensor)] in the order of `plan`"""
    return SimpleNamespace(all=[], **{r: Formats(wslot) for r in ROLES})
