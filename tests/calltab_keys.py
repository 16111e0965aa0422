"""The call-name table's hash (csrc/calls_core.h: FNV-1a over the bytes, then
murmur3's 64-bit finalizer; home slot = hash & (nslots - 1), nslots the least
power of two >= 2 n, at least 2) restated, and names brute-forced onto one home
slot for the table tests."""
M64 = (1 << 64) - 1


def fmix64(k):
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & M64
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & M64
    k ^= k >> 33
    return k


def name_hash(name):
    h = 0xCBF29CE484222325
    for b in name:
        h = (h ^ b) * 0x100000001B3 & M64
    return fmix64(h)


def slots_for(n):
    s = 2
    while s < 2 * n:
        s <<= 1
    return s


def home(name, nslots):
    return name_hash(name) & (nslots - 1)


def colliding_names(count, nslots, slot=0, prefix=b"sys_"):
    """`count` distinct identifier names whose home slot in a table of nslots is `slot`."""
    out, k = [], 0
    while len(out) < count:
        nm = prefix + b"%d" % k
        if home(nm, nslots) == slot:
            out.append(nm)
        k += 1
    return out


def absent_name(names, nslots, slot=0, prefix=b"absent_"):
    """A name on the same home slot that is none of `names`."""
    have, k = set(names), 0
    while True:
        nm = prefix + b"%d" % k
        if nm not in have and home(nm, nslots) == slot:
            return nm
        k += 1
