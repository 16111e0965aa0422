"""Comparison hints on device: prog.CompMap (prog/hints.go:27-48) for every
call of a batch, prog.shrinkExpand (hints.go:164-218) against it, and the
mutants of checkConstArg / checkDataArg (hints.go:105-132) for a batch of args.

A CompMap holds the maps of a batch's calls as CSR over device tensors: call
c's distinct (key, value) pairs, sorted ascending by key, then value (as
unsigned 64-bit words; one fixed instance of Go's map order), at
pairs[off[c]:off[c + 1]].  Everything is computed by libsyzsig's kernels
(csrc/comps.hip, csrc/hints.hip); torch owns the buffers.
"""
import torch

from . import _lib

__all__ = ["CompMap", "SPECIAL_INTS", "apply_mutant"]

# prog/rand.go:57-65 specialInts: the caller's list, handed to shrink_expand
# (the library hard-codes none)
SPECIAL_INTS = (0, 1, 31, 32, 63, 64, 127, 128, 129, 255, 256, 257, 511, 512, 1023, 1024, 1025, 2047, 2048, 4095, 4096,
                (1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 16) - 1, 1 << 16, (1 << 16) + 1,
                (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1)


def _u64(x):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x  # as torch's int64 holds it


def apply_mutant(data, at, nb, rep):
    """hints.go:126-127 on the host: `data` with its bytes at .. at + nb set to
    the low nb bytes of rep, little-endian (nb = min(8, len(data) - at), as
    mutate_with_hints reports it)."""
    at, nb = int(at), int(nb)
    if not (0 <= at and 0 <= nb <= 8 and at + nb <= len(data)):
        raise ValueError("mutant outside the arg")
    b = (int(rep) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
    return bytes(data[:at]) + b[:nb] + bytes(data[at + nb:])


class CompMap:
    def __init__(self, dev, status, off, pairs):
        self.dev, self.status, self.off, self.pairs = dev, status, off, pairs

    @property
    def ncalls(self):
        return self.off.numel() - 1

    @classmethod
    def from_exec_output(cls, dev, words, call_start, out_words, comps_cnt):
        """From Device.exec_comps' output: call c's comps_cnt[c] records at
        words[5 * call_start[c] : +out_words[c]]."""
        start = (5 * call_start.to(torch.int64)).contiguous()
        end = (start + out_words.to(torch.int64)).contiguous()
        return cls(dev, *dev.comp_map(words, start, comps_cnt, end))

    @classmethod
    def from_regions(cls, dev, out, ingest_result):
        """From executor output regions and what Device.ingest_exec_output(...,
        want_cover=True) returned for them.  For an executed call (Errno != -1;
        every call of a program that failed to parse has -1) the comparisons
        follow its cover (comps_start = cover_start + cover_len) and compsSize
        is the header word before its signal (out[call_start - 1]); every other
        call has none.  The ingest walked these records already, so they lie
        inside their program's region."""
        r = ingest_result
        executed = (r["call_errno"] != -1) & (out.numel() > 0)
        zero = torch.zeros((), dtype=torch.int64, device=dev.dev)
        start = torch.where(executed, r["cover_start"] + r["cover_len"].to(torch.int64), zero)
        hdr = torch.where(executed, r["call_start"] - 1, zero)
        cnt = torch.where(executed, out[hdr].to(torch.int64) if out.numel() else zero, zero).to(torch.int32)
        return cls(dev, *dev.comp_map(out, start.contiguous(), cnt.contiguous()))

    def lookup(self, call, key):
        """compMap[key] of call `call`: its values as a sorted list of ints."""
        o = self.off[call:call + 2].cpu().tolist()
        p = self.pairs[o[0]:o[1]]
        v = p[p[:, 0] == _u64(key), 1].cpu().tolist()
        return sorted(int(x) & 0xFFFFFFFFFFFFFFFF for x in v)

    def shrink_expand(self, calls, values, special_ints=SPECIAL_INTS):
        """shrinkExpand(values[q], maps[calls[q]]) for every query -> (rep_off
        int64[nq + 1], rep int64[total]), query q's replacers sorted."""
        calls = torch.as_tensor(calls, dtype=torch.int32, device=self.dev.dev).contiguous()
        if not torch.is_tensor(values):
            values = torch.tensor([_u64(v) for v in values], dtype=torch.int64)
        values = values.to(self.dev.dev, torch.int64).contiguous()
        return self.dev.shrink_expand(self.off, self.pairs, calls, values, special_ints)

    def mutate_with_hints(self, arg_call, arg_kind, arg_val, arg_off, data, special_ints=SPECIAL_INTS):
        """checkConstArg / checkDataArg (hints.go:105-132) for every arg of a
        batch; the caller has applied generateHints' type filter (:83-95).
        arg_call[a] = the call whose map arg a is matched against, arg_kind[a]
        = 0 (ConstArg: arg_val[a]) or 1 (DataArg: data[arg_off[a]:arg_off[a +
        1]]).  Returns (mut_off int64[narg + 1], at int32[total], nb
        uint8[total], rep int64[total]): a ConstArg's mutants are (0, 8, its
        new Val), a DataArg's are what apply_mutant takes."""
        d = self.dev.dev
        arg_call = torch.as_tensor(arg_call, dtype=torch.int32, device=d).contiguous()
        arg_kind = torch.as_tensor(arg_kind, dtype=torch.uint8, device=d).contiguous()
        if not torch.is_tensor(arg_val):
            arg_val = torch.tensor([_u64(v) for v in arg_val], dtype=torch.int64)
        arg_val = arg_val.to(d, torch.int64).contiguous()
        arg_off = torch.as_tensor(arg_off, dtype=torch.int64, device=d).contiguous()
        if not torch.is_tensor(data):
            data = torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8)
        data = data.to(d, torch.uint8).contiguous()
        return self.dev.hint_mutants(self.off, self.pairs, arg_call, arg_kind, arg_val, arg_off, data, special_ints)
