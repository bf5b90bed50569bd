"""No-GPU checks of the TFRecord shard reader (rd_tfrecord_*, radian_amd/tfrecord.py): crc32c, shards written by an independent
protobuf-descriptor encoder (tests/_tfrecord_writer.py) read back exactly in packed and unpacked form, every refusal naming its
record, and an ASan / UBSan build of the parser on truncated and corrupted shards."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _tfrecord_writer as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tfr():
    from radian_amd import build
    build.build()
    from radian_amd import tfrecord
    return tfrecord


def _records(rng, n, max_label=63, pad_to=None):
    out = []
    for _ in range(n):
        sl = int(rng.integers(1, 1025))
        ll = int(rng.integers(0, max_label + 1))
        lab = rng.integers(0, 4, size=ll).astype(float).tolist()
        if pad_to is not None:
            lab += [0.0] * (pad_to - ll)    # Keras-style padding past label_length
        out.append((rng.normal(size=1024).astype(np.float32), lab, sl, ll))
    return out


def test_crc32c_known_vectors(tfr):
    assert tfr.crc32c(b"123456789") == 0xE3069283
    assert tfr.crc32c(b"") == 0
    assert tfr.crc32c(bytes(32)) == 0x8A9136AA          # RFC 3720 B.4: 32 bytes of zeros
    assert tfr.crc32c(b"\xff" * 32) == 0x62A8AB43        # ... and of ones
    rng = np.random.default_rng(1)
    for n in (1, 7, 8, 9, 63, 1000):
        b = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert tfr.crc32c(b) == tw.crc32c(b)


@pytest.mark.parametrize("packed", [True, False])
def test_shards_of_an_independent_encoder_read_back_exactly(tfr, tmp_path, packed):
    rng = np.random.default_rng(2 if packed else 3)
    recs = _records(rng, 40, max_label=255, pad_to=None) + _records(rng, 20, max_label=25, pad_to=25)
    recs.append((np.arange(1024, dtype=np.float32), [], 1024, 0))
    recs.append((np.full(1024, -0.0, dtype=np.float32), [3.0] * 255, 1, 255))
    p = tmp_path / "s.tfrecords"
    tw.write_shard(p, recs, packed=packed)
    sh = tfr.read_shard(p)
    assert len(sh) == len(recs)
    for i, (sig, lab, sl, ll) in enumerate(recs):
        assert sh.signals[i].tobytes() == np.asarray(sig, dtype=np.float32).tobytes()
        assert sh.input_len[i] == sl and sh.label_len[i] == ll
        assert sh.label(i).tolist() == [int(v) for v in lab[:ll]]
    same = tfr.read_shard_bytes(p.read_bytes())
    assert same.signals.tobytes() == sh.signals.tobytes() and same.labels.tobytes() == sh.labels.tobytes()


def test_field_order_unknown_fields_and_overrides(tfr):
    # extra features, a bytes feature, and a key given twice (the last wins) are accepted
    sig = np.ones(1024, dtype=np.float32)
    ex = tw.example_bytes(sig, [1, 2], 5, 2, extra={"other": ("bytes", [b"xyz"]), "n": ("int64", [7, 8])})
    sh = tfr.read_shard_bytes(tw.frame(ex))
    assert sh.label(0).tolist() == [1, 2] and sh.input_len[0] == 5
    # Features repeated: protobuf merges the map, the later entry of a key wins
    later = tw.example_bytes(sig, [3], 9, 1, drop=("signal",))
    sh = tfr.read_shard_bytes(tw.frame(ex + later))
    assert sh.label(0).tolist() == [3] and sh.input_len[0] == 9 and sh.signals[0].tolist() == sig.tolist()
    assert len(tfr.read_shard_bytes(b"")) == 0


def _refused(tfr, data, *words):
    with pytest.raises(tfr.TFRecordError) as e:
        tfr.read_shard_bytes(data)
    msg = str(e.value)
    for w in words:
        assert w in msg, msg
    return msg


def test_every_refusal_names_its_record(tfr):
    sig = np.zeros(1024, dtype=np.float32)
    good = tw.frame(tw.example_bytes(sig, [0, 1], 10, 2))
    pre = good * 3   # records 0..2 are fine: the bad one is record 3

    def bad(**kw):
        a = dict(signal=sig, label=[0, 1], signal_length=10, label_length=2)
        a.update(kw)
        return pre + tw.frame(tw.example_bytes(a["signal"], a["label"], a["signal_length"], a["label_length"], drop=kw.get("_drop", ())))

    _refused(tfr, bad(signal_length=0), "record 3", "signal_length 0")
    _refused(tfr, bad(signal_length=1025), "record 3", "signal_length 1025")
    _refused(tfr, bad(label_length=3), "record 3", "label_length 3")
    _refused(tfr, bad(label_length=-1), "record 3", "label_length -1")
    _refused(tfr, bad(label=[0, 4]), "record 3", "label 1 is 4")
    _refused(tfr, bad(label=[0.5, 1]), "record 3", "label 0 is 0.5")
    _refused(tfr, bad(signal=np.zeros(1023, dtype=np.float32)), "record 3", "1023 values")
    for f in ("signal", "label", "signal_length", "label_length"):
        data = pre + tw.frame(tw.example_bytes(sig, [0, 1], 10, 2, drop=(f,)))
        _refused(tfr, data, "record 3", f"'{f}' is missing")
    data = pre + tw.frame(tw.example_bytes(sig, [0, 1], 10, 2, extra={"label": ("int64", [0, 1])}))
    _refused(tfr, data, "record 3", "not a float list")
    # framing: a flipped data byte, a flipped length byte, truncation anywhere in the last frame
    last = bytearray(tw.frame(tw.example_bytes(sig, [0, 1], 10, 2)))
    d = bytearray(last)
    d[40] ^= 1
    _refused(tfr, pre + bytes(d), "record 3", "data checksum")
    d = bytearray(last)
    d[1] ^= 1
    _refused(tfr, pre + bytes(d), "record 3", "length checksum")
    d = bytearray(last)
    d[-1] ^= 0x80
    _refused(tfr, pre + bytes(d), "record 3", "data checksum")
    for cut in (1, 11, 12, 13, len(last) - 5, len(last) - 1):
        _refused(tfr, pre + bytes(last[:cut]), "record 3", "truncated")
    # a frame whose checksums are right around a message that is cut short
    body = tw.example_bytes(sig, [0, 1], 10, 2)[:-3]
    _refused(tfr, pre + tw.frame(body), "record 3")


def test_file_errors(tfr, tmp_path):
    with pytest.raises(OSError):
        tfr.read_shard(tmp_path / "absent.tfrecords")
    p = tmp_path / "bad.tfrecords"
    p.write_bytes(b"\x01" * 20)
    msg = _refused(tfr, b"\x01" * 20, "record 0")
    with pytest.raises(tfr.TFRecordError) as e:
        tfr.read_shard(p)
    assert "record 0" in str(e.value) and str(p) in str(e.value), msg


def test_asan_parser_on_truncated_and_corrupted_shards(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    rng = np.random.default_rng(4)
    p1, p2 = tmp_path / "packed.tfrecords", tmp_path / "unpacked.tfrecords"
    tw.write_shard(p1, _records(rng, 6, max_label=40, pad_to=40), packed=True)
    tw.write_shard(p2, _records(rng, 6, max_label=40), packed=False)
    exe = tmp_path / "asan_tfrecord"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "radian_amd", "csrc", "tfrecord.hip"),
                        os.path.join(ROOT, "tests", "asan_tfrecord.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "1500", str(p1), str(p2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    lines = r.stdout.decode().splitlines()
    assert lines[0].endswith(": 6 records") and lines[1].endswith(": 6 records")
    opened, refused = int(lines[-1].split()[0]), int(lines[-1].split()[2])
    assert opened > 100 and refused > 1000          # the mutations reach both outcomes
