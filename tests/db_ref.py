"""pkg/db/db.go restated for the tests: deserializeDB / deserializeHeader /
deserializeRecord (:177-265) over a file's bytes with zlib.decompressobj(-15) as
flate.NewReader, and serializeHeader / serializeRecord (:141-175) with the stream
shape of Go's flate.Writer Write + Flush + Close (the data's blocks, an empty
stored block, an empty final stored block).  No device, no library."""
import struct
import zlib

DB_MAGIC = 0xBADDB
REC_MAGIC = 0xFEE1BAD
CUR_VERSION = 2
SEQ_DELETED = (1 << 64) - 1

# how a replay ended
EOF, BAD_HEADER, BAD_MAGIC, TRUNCATED, INFLATE, TRAILING = "eof", "bad_header", "bad_magic", "truncated", "inflate", "trailing"
# inflate classes (the names of SYZSIG_INFLATE_*)
OK, S_TRUNCATED, S_INVALID, S_TRAILING, S_TOO_LONG = range(5)


class RecordError(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def inflate_class(stream):
    """(class, bytes) of one raw DEFLATE stream as zlib sees it: zlib.error is
    INVALID, eof not reached TRUNCATED, bytes after the final block TRAILING."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream))
    except zlib.error:
        return S_INVALID, b""
    if not d.eof:
        return S_TRUNCATED, b""
    if d.unused_data:
        return S_TRAILING, b""
    return OK, out


def go_stream(val, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
    """fw.Write(val); fw.Flush(); fw.Close() (db.go:164-172)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(bytes(val)) + c.flush(zlib.Z_SYNC_FLUSH) + b"\x01\x00\x00\xff\xff"


def stored_stream(val):
    """val as stored blocks alone, in the same shape: no compressor involved."""
    out = b""
    for i in range(0, len(val), 65535):
        chunk = val[i:i + 65535]
        out += b"\x00" + struct.pack("<HH", len(chunk), len(chunk) ^ 0xFFFF) + chunk
    return out + b"\x00\x00\x00\xff\xff" + b"\x01\x00\x00\xff\xff"


def serialize_header(version, ver=CUR_VERSION):
    """:141-145 (ver = 1: the old header without the user version)."""
    return struct.pack("<II", DB_MAGIC, ver) + (struct.pack("<Q", version) if ver >= 2 else b"")


def serialize_record(key, val, seq, stream=go_stream):
    """:147-175.  key: bytes."""
    out = struct.pack("<II", REC_MAGIC, len(key)) + bytes(key) + struct.pack("<Q", seq)
    if seq == SEQ_DELETED:
        assert not val, "deleting record with value"
        return out
    if len(val) == 0:
        return out + struct.pack("<I", 0)
    body = stream(val)
    return out + struct.pack("<I", len(body)) + body


def serialize_db(version, records, stream=go_stream):
    """records: (key, val, seq) in file order; seq == SEQ_DELETED is a delete."""
    return serialize_header(version) + b"".join(serialize_record(k, v, s, stream) for k, v, s in records)


class _Reader:
    def __init__(self, data):
        self.d, self.at = bytes(data), 0

    def read(self, n, at_boundary=False):
        """binary.Read / io.ReadFull: io.EOF only with nothing read"""
        left = len(self.d) - self.at
        if left == 0 and at_boundary:
            raise EOFError
        if left < n:
            raise RecordError(TRUNCATED)
        self.at += n
        return self.d[self.at - n:self.at]


def deserialize_header(r):
    """:203-227 -> user version"""
    try:
        magic, = struct.unpack("<I", r.read(4, at_boundary=True))
    except EOFError:
        return 0
    if magic != DB_MAGIC:
        raise RecordError(BAD_HEADER)
    ver, = struct.unpack("<I", r.read(4))
    if ver == 0 or ver > CUR_VERSION:
        raise RecordError(BAD_HEADER)
    user = 0
    if ver >= 2:
        user, = struct.unpack("<Q", r.read(8))
    return user


def deserialize_record(r):
    """:229-265 -> (key, val, seq); EOFError at a record boundary"""
    magic, = struct.unpack("<I", r.read(4, at_boundary=True))
    if magic != REC_MAGIC:
        raise RecordError(BAD_MAGIC)
    key_len, = struct.unpack("<I", r.read(4))
    key = r.read(key_len)
    seq, = struct.unpack("<Q", r.read(8))
    if seq == SEQ_DELETED:
        return key, None, seq
    val_len, = struct.unpack("<I", r.read(4))
    val = b""
    if val_len != 0:
        # io.LimitedReader{r, valLen}: a value that runs past the file's end is the file ending inside
        # the record, whatever its bytes are
        cls, val = inflate_class(r.read(val_len))
        if cls == S_TRAILING:
            raise RecordError(TRAILING)  # this project's class: the reference's answer is not defined
        if cls != OK:
            raise RecordError(INFLATE)
    return key, val, seq


def deserialize_db(data):
    """:177-200 -> (version, records {key: (val, seq)}, uncompacted, ended)"""
    r = _Reader(data)
    records = {}
    try:
        version = deserialize_header(r)
    except RecordError:
        return 0, records, 0, BAD_HEADER  # (a header cut short is a bad header too)
    uncompacted = 0
    while True:
        try:
            key, val, seq = deserialize_record(r)
        except EOFError:
            return version, records, uncompacted, EOF
        except RecordError as e:
            return version, records, uncompacted, e.kind
        uncompacted += 1
        if seq == SEQ_DELETED:
            records.pop(key, None)
        else:
            records[key] = (val, seq)


def needs_compact(nrecords, uncompacted):
    """:49"""
    return nrecords == 0 or uncompacted // 10 * 9 > nrecords
