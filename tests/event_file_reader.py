"""An independent reader of TensorBoard event files for the tests of training/summary.py: TFRecord framing checked with a bitwise CRC-32C
written here, messages decoded by google.protobuf classes built at run time from a FileDescriptorProto that spells out the field numbers
(no generated code, nothing shared with the writer under test)."""
import io
import struct

import numpy as np


def crc32c_bitwise(data, crc=0):
    """CRC-32C (Castagnoli), reflected polynomial 0x82F63B78, one bit at a time"""
    c = crc ^ 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def crc32c_table(data):
    """the same function a byte at a time, for payloads of megabytes (checked against the bitwise form in the tests)"""
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        table.append(c)
    c = 0xFFFFFFFF
    for b in data:
        c = (c >> 8) ^ table[(c ^ b) & 0xFF]
    return c ^ 0xFFFFFFFF


def masked(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def records(path, crc=crc32c_bitwise):
    """the payloads of a file of TFRecords; every length and payload checksum is recomputed"""
    data = open(path, "rb").read()
    out, at = [], 0
    while at < len(data):
        assert at + 12 <= len(data), "truncated record header at byte %d" % at
        (length,) = struct.unpack_from("<Q", data, at)
        (len_crc,) = struct.unpack_from("<I", data, at + 8)
        assert len_crc == masked(crc(data[at:at + 8])), "length checksum at byte %d" % at
        assert at + 12 + length + 4 <= len(data), "truncated payload at byte %d" % at
        payload = data[at + 12:at + 12 + length]
        (pay_crc,) = struct.unpack_from("<I", data, at + 12 + length)
        assert pay_crc == masked(crc(payload)), "payload checksum at byte %d" % at
        out.append(payload)
        at += 12 + length + 4
    return out


_classes = {}


def message_classes():
    """-> dict of the four message classes, built from a descriptor written out here"""
    if _classes:
        return _classes
    from google.protobuf import descriptor_pb2, descriptor_pool
    try:
        from google.protobuf.message_factory import GetMessageClass
    except ImportError:                                  # older protobuf
        from google.protobuf import message_factory
        GetMessageClass = lambda d: message_factory.MessageFactory().GetPrototype(d)
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="footprints_test_event.proto", package="fptest", syntax="proto2")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, type_name in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if type_name:
                f.type_name = ".fptest." + type_name
    opt, rep = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg("Image", [("height", 1, F.TYPE_INT32, opt, None), ("width", 2, F.TYPE_INT32, opt, None), ("colorspace", 3, F.TYPE_INT32, opt, None),
                  ("encoded_image_string", 4, F.TYPE_BYTES, opt, None)])
    msg("Value", [("tag", 1, F.TYPE_STRING, opt, None), ("simple_value", 2, F.TYPE_FLOAT, opt, None), ("image", 4, F.TYPE_MESSAGE, opt, "Image")])
    msg("Summary", [("value", 1, F.TYPE_MESSAGE, rep, "Value")])
    msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, opt, None), ("step", 2, F.TYPE_INT64, opt, None), ("file_version", 3, F.TYPE_STRING, opt, None),
                  ("summary", 5, F.TYPE_MESSAGE, opt, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    for name in ("Image", "Value", "Summary", "Event"):
        _classes[name] = GetMessageClass(pool.FindMessageTypeByName("fptest." + name))
    return _classes


def events(path, crc=crc32c_bitwise):
    """-> the file's Event messages; each must serialise back to the bytes it was parsed from"""
    Event = message_classes()["Event"]
    out = []
    for payload in records(path, crc):
        ev = Event()
        ev.ParseFromString(payload)
        assert ev.SerializeToString() == payload, "a non-canonical encoding"
        out.append(ev)
    return out


def decode_png(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "PNG" and im.mode == "RGB", (im.format, im.mode)
        return np.asarray(im, dtype=np.uint8)


def read_log(path, crc=crc32c_table):
    """-> (version string of the first record, [(step, tag, float | uint8 [H, W, 3])] of every later record's single value)"""
    evs = events(path, crc)
    assert evs and evs[0].file_version == "brain.Event:2" and len(evs[0].summary.value) == 0, "the first record must be the version"
    out = []
    for ev in evs[1:]:
        assert ev.file_version == "" and len(ev.summary.value) == 1 and ev.wall_time > 1e9, "one value per event"
        v = ev.summary.value[0]
        if v.HasField("image"):
            pic = decode_png(v.image.encoded_image_string)
            assert (v.image.height, v.image.width, v.image.colorspace) == (pic.shape[0], pic.shape[1], 3)
            out.append((ev.step, v.tag, pic))
        else:
            out.append((ev.step, v.tag, v.simple_value))
    return evs[0].file_version, out
