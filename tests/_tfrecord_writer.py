"""An encoder of TFRecord shards of tf.train.Example records, independent of the library's reader: the messages are built from
google.protobuf descriptors of example.proto / feature.proto (declared here; TensorFlow is not needed) and framed with a
crc32c written out bit by bit.  Test infrastructure (tests/test_tfrecord_cpu.py, tests/test_gpu_ctc.py)."""
import struct

from google.protobuf import descriptor_pb2, descriptor_pool, message_factory


def _crc32c_bitwise(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def crc32c(data):
    return _crc32c_bitwise(data)


def masked_crc(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _classes(packed):
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name=f"example_{int(packed)}.proto", package=f"t{int(packed)}", syntax="proto3")

    def msg(name, fields, nested=()):
        m = fd.message_type.add(name=name)
        for fname, num, typ, label, tname, opts in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if tname:
                f.type_name = tname
            if opts is not None:
                f.options.packed = opts
        for n in nested:
            m.nested_type.add().CopyFrom(n)
        return m

    R, O = F.LABEL_REPEATED, F.LABEL_OPTIONAL
    p = f".t{int(packed)}."
    msg("BytesList", [("value", 1, F.TYPE_BYTES, R, None, None)])
    msg("FloatList", [("value", 1, F.TYPE_FLOAT, R, None, packed)])
    msg("Int64List", [("value", 1, F.TYPE_INT64, R, None, packed)])
    feat = msg("Feature", [("bytes_list", 1, F.TYPE_MESSAGE, O, p + "BytesList", None), ("float_list", 2, F.TYPE_MESSAGE, O, p + "FloatList", None),
                           ("int64_list", 3, F.TYPE_MESSAGE, O, p + "Int64List", None)])
    feat.oneof_decl.add(name="kind")
    for f in feat.field:
        f.oneof_index = 0
    entry = descriptor_pb2.DescriptorProto(name="FeatureEntry")
    entry.field.add(name="key", number=1, type=F.TYPE_STRING, label=O)
    entry.field.add(name="value", number=2, type=F.TYPE_MESSAGE, label=O, type_name=p + "Feature")
    entry.options.map_entry = True
    msg("Features", [("feature", 1, F.TYPE_MESSAGE, R, p + "Features.FeatureEntry", None)], nested=[entry])
    msg("Example", [("features", 1, F.TYPE_MESSAGE, O, p + "Features", None)])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName(f"t{int(packed)}.Example"))


_EXAMPLE = {}


def example_bytes(signal, label, signal_length, label_length, packed=True, extra=None, drop=()):
    """a serialised tf.train.Example with the four features of radian/data.py:9-15 (a feature named in drop is left out; extra:
    {name: ("float" | "int64" | "bytes", values)} added)"""
    if packed not in _EXAMPLE:
        _EXAMPLE[packed] = _classes(packed)
    ex = _EXAMPLE[packed]()
    feats = {"signal": ("float", signal), "label": ("float", label), "signal_length": ("int64", [signal_length]),
             "label_length": ("int64", [label_length])}
    feats.update(extra or {})
    for name, (kind, vals) in feats.items():
        if name in drop:
            continue
        f = ex.features.feature[name]
        if kind == "float":
            f.float_list.value.extend(float(v) for v in vals)
        elif kind == "int64":
            f.int64_list.value.extend(int(v) for v in vals)
        else:
            f.bytes_list.value.extend(bytes(v) for v in vals)
    return ex.SerializeToString()


def frame(data):
    n = struct.pack("<Q", len(data))
    return n + struct.pack("<I", masked_crc(n)) + data + struct.pack("<I", masked_crc(data))


def write_shard(path, records, packed=True):
    """records: [(signal [1024], label list, signal_length, label_length)]"""
    with open(path, "wb") as f:
        for r in records:
            f.write(frame(example_bytes(*r, packed=packed)))
