"""TensorBoard event files, written without a TensorBoard package: `SummaryWriter(logdir)` with the four methods the trainer uses.

The reference logs through tensorboardX (training/train.py:47-50, training/logger.py); neither it nor torch.utils.tensorboard can be
assumed here, so the file format is written out by hand.  An event file is a sequence of TFRecords,

    u64 little-endian length | u32 masked CRC-32C of those eight bytes | payload | u32 masked CRC-32C of the payload

with masked(crc) = ((crc >> 15 | crc << 17) + 0xa282ead8) mod 2^32, and every payload a protobuf `Event`:

    Event    wall_time = 1 (double)   step = 2 (int64)   file_version = 3 (string)   summary = 5 (Summary)
    Summary  value = 1 (repeated Value)
    Value    tag = 1 (string)   simple_value = 2 (float)   image = 4 (Image)
    Image    height = 1   width = 2   colorspace = 3   encoded_image_string = 4 (bytes)

The first record carries file_version "brain.Event:2"; after it one Event per add_* call, as tensorboardX writes them.  The CRC is the
library's fp_crc32c through ctypes, which lets go of the interpreter lock for the megabytes of PNG of a log event; a process that cannot
load the library falls back on a table-driven loop in Python with the same results."""
import io
import os
import socket
import struct
import time

_CRC_TABLE = None


def crc32c_python(data, crc=0):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of `data`, continuing from `crc`: the fallback of `crc32c`"""
    global _CRC_TABLE
    if _CRC_TABLE is None:
        table = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            table.append(c)
        _CRC_TABLE = table
    table, c = _CRC_TABLE, crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = (c >> 8) ^ table[(c ^ b) & 0xFF]
    return c ^ 0xFFFFFFFF


_native = []        # [fp_crc32c or None] once looked up


def _native_crc():
    if not _native:
        try:
            from .. import _lib
            _native.append(_lib.load().fp_crc32c)
        except (RuntimeError, OSError, AttributeError):
            _native.append(None)
    return _native[0]


def crc32c(data, crc=0):
    """CRC-32C of a bytes-like object, continuing from `crc` (0 at the start)"""
    fn = _native_crc()
    if fn is None:
        return crc32c_python(data, crc)
    data = bytes(data)
    return int(fn(crc, data, len(data)))


def masked_crc(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---- protobuf wire format: varints, and fields of wire types 0 (varint), 1 (64-bit), 2 (length-delimited), 5 (32-bit) ---------------------
def _varint(v):
    v &= (1 << 64) - 1                       # int64 fields: two's complement, ten bytes for a negative value
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _key(field, wire):
    return _varint(field << 3 | wire)


def _bytes_field(field, payload):
    return _key(field, 2) + _varint(len(payload)) + payload


def _varint_field(field, v):
    return _key(field, 0) + _varint(int(v))


def encode_event(wall_time, step=None, file_version=None, summary=None):
    out = _key(1, 1) + struct.pack("<d", float(wall_time))
    if step is not None:
        out += _varint_field(2, step)
    if file_version is not None:
        out += _bytes_field(3, file_version.encode("utf-8"))
    if summary is not None:
        out += _bytes_field(5, summary)
    return out


def encode_scalar_summary(tag, value):
    val = _bytes_field(1, tag.encode("utf-8")) + _key(2, 5) + struct.pack("<f", float(value))
    return _bytes_field(1, val)


def encode_image_summary(tag, height, width, png):
    img = _varint_field(1, height) + _varint_field(2, width) + _varint_field(3, 3) + _bytes_field(4, png)
    return _bytes_field(1, _bytes_field(1, tag.encode("utf-8")) + _bytes_field(4, img))


def encode_png(rgb):
    """uint8 [H, W, 3] -> PNG bytes, with Pillow as tensorboardX's make_image encodes them"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    return buf.getvalue()


class SummaryWriter:
    """`events.out.tfevents.<unix seconds>.<hostname>` under logdir (created if missing); records are buffered by the file object until
    `flush` or `close`"""

    def __init__(self, logdir, encode_png=encode_png):
        os.makedirs(logdir, exist_ok=True)
        self.logdir = logdir
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(time.time()), socket.gethostname()))
        self.encode_png = encode_png
        self._fh = open(self.path, "ab")
        self._record(encode_event(time.time(), file_version="brain.Event:2"))
        self.flush()

    def _record(self, payload):
        if self._fh is None:
            raise ValueError("SummaryWriter: %s is closed" % self.path)
        head = struct.pack("<Q", len(payload))
        self._fh.write(head + struct.pack("<I", masked_crc(head)) + payload + struct.pack("<I", masked_crc(payload)))

    def add_scalar(self, tag, value, step, walltime=None):
        self._record(encode_event(time.time() if walltime is None else walltime, step=step, summary=encode_scalar_summary(tag, value)))

    def add_image(self, tag, rgb_uint8_hwc, step, walltime=None):
        """rgb_uint8_hwc: numpy uint8 [H, W, 3]"""
        import numpy as np
        rgb = np.ascontiguousarray(rgb_uint8_hwc)
        if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("SummaryWriter.add_image: %s must be uint8 [H, W, 3], got %s %r" % (tag, rgb.dtype, rgb.shape))
        summary = encode_image_summary(tag, rgb.shape[0], rgb.shape[1], self.encode_png(rgb))
        self._record(encode_event(time.time() if walltime is None else walltime, step=step, summary=summary))

    def flush(self):
        if self._fh is not None:
            self._fh.flush()

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None
