"""pkg/db/db.go's write side restated for the tests, line by line: Save (:55-65),
Delete (:67-74), Flush (:76-94), BumpVersion (:96-102), compact (:104-125) and
serialize (:127-132) over an ordered dict and a log of (key, val, seq).  The
stream function is pluggable (db_ref.go_stream is Go's shape); the frames are
db_ref.serialize_record's.  Files are the caller's here as in the library:
flush / compact return the bytes the reference would write.  No device."""
from tests import db_ref as R

SEQ_DELETED = R.SEQ_DELETED


class RefDB:
    def __init__(self, version=0, records=None, uncompacted=None, stream=R.go_stream):
        """records: {key: (val, seq)} in file order of the last write (what
        db_ref.deserialize_db returns)."""
        self.version = version
        self.records = dict(records or {})
        self.uncompacted = len(self.records) if uncompacted is None else uncompacted
        self.pending = None  # bytes, or None (db.pending == nil)
        self.log = []        # every (key, val, seq) that reached serialize, over the DB's life
        self.stream = stream

    @classmethod
    def open(cls, data, stream=R.go_stream):
        """deserializeDB without Open's compact (the library's open_db does not compact either)"""
        version, records, uncompacted, _ = R.deserialize_db(data)
        return cls(version, records, uncompacted, stream)

    def save(self, key, val, seq):
        val = bytes(val or b"")
        if seq == SEQ_DELETED:
            raise ValueError("reserved seq")                       # :56-58
        rec = self.records.get(key)
        if rec is not None and seq == rec[1] and val == rec[0]:    # :59-61
            return
        self.records.pop(key, None)  # (the dict keeps the order of the last writes, as a reopened file has it)
        self.records[key] = (val, seq)                             # :62
        self.serialize(key, val, seq)                              # :63
        self.uncompacted += 1                                      # :64

    def delete(self, key):
        if key not in self.records:                                # :68-70
            return
        del self.records[key]                                      # :71
        self.serialize(key, None, SEQ_DELETED)                     # :72
        self.uncompacted += 1                                      # :73

    def apply(self, ops):
        """(key, val, seq) in order; seq == ^0 is a Delete"""
        for key, val, seq in ops:
            if seq == SEQ_DELETED:
                assert not val, "deleting record with value"
                self.delete(key)
            else:
                self.save(key, val, seq)

    def flush(self):
        if self.uncompacted // 10 * 9 > len(self.records):         # :77-80
            return "replace", self.compact()
        if self.pending is None:                                   # :81-83
            return None
        out, self.pending = self.pending, None                     # :89-92
        return "append", out

    def bump_version(self, version):
        if self.version == version:                                # :97-99
            return self.flush()
        self.version = version                                     # :100
        return "replace", self.compact()                           # :101

    def compact(self):
        out = R.serialize_header(self.version)                     # :106
        for key, (val, seq) in self.records.items():               # :107-109 (map order there; file order here)
            out += R.serialize_record(key, val, seq, self.stream)
        self.uncompacted = len(self.records)                       # :122
        self.pending = None                                        # :123
        return out

    def serialize(self, key, val, seq):
        if self.pending is None:                                   # :128-130
            self.pending = b""
        self.pending += R.serialize_record(key, val, seq, self.stream)  # :131
        self.log.append((key, val, seq))
