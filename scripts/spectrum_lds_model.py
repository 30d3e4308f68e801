"""LDS bank model of the sample-spectrum kernel (csrc/gat_spec.hip): for every transform size, every LDS
access of one segment -- the bit-reversed staging stores, each pass's reads and write-backs, the twiddle reads -- is laid over
the banks by the rule of the hardware (8-byte reads: groups of 32 lanes on 64 dword banks; 8-byte stores: groups of 16 lanes on
32 dword banks; equal addresses broadcast), and the LDS cycles are counted against the conflict-free count.  The index maps are
restated here from gat_spec_plan.h; `--map` tries another skew of the point and twiddle arrays.

    python scripts/spectrum_lds_model.py            # the maps the kernel uses
    python scripts/spectrum_lds_model.py --map none # what plain power-of-two strides would cost
"""
from __future__ import annotations

import argparse

THREADS = 256


def fold(p):  # the kernel's skew: the low five bits XORed with the next two five-bit digits (spec_skew)
    return p ^ ((p >> 5) & 31) ^ ((p >> 10) & 31)


def pad(p):
    return p + (p >> 5)


def pad2(p):
    return p + (p >> 5) + (p >> 10)


MAPS = {"none": lambda p: p, "fold": fold, "pad": pad, "pad2": pad2}


def bitrev(n, L):
    return int(format(n, f"0{L}b")[::-1], 2)


def geometry(F):
    L = F.bit_length() - 1
    R = max(4, F // THREADS)
    r = R.bit_length() - 1
    team = F // R
    passes = -(-L // r)
    r0 = L - r * (passes - 1)
    return L, R, r, team, THREADS // team, passes, r0


def point_index(t, i, R, j, rs):
    v = t * (R >> rs) + (i >> rs)
    ii = i & ((1 << rs) - 1)
    return ((v >> j) << (j + rs)) | (ii << j) | (v & ((1 << j) - 1)), v, ii


def cycles(addrs, group, banks):
    """LDS cycles of one wave instruction: per lane group, the most distinct addresses on one bank"""
    total = 0
    for g0 in range(0, len(addrs), group):
        per = {}
        for a in set(addrs[g0:g0 + group]):
            per.setdefault(a % banks, set()).add(a)
        total += max(len(v) for v in per.values())
    return total


def model(F, pmap, tmap, vs):
    L, R, r, team, teams, passes, r0 = geometry(F)
    pitch = max(pmap(p) for p in range(F)) + 1
    out = {"stage": [0, 0], "read": [0, 0], "write": [0, 0], "twiddle": [0, 0]}

    def add(kind, per_lane, group, banks):
        for w0 in range(0, THREADS, 64):
            a = [per_lane(l) for l in range(w0, w0 + 64)]
            a = [x for x in a if x is not None]
            if not a:
                continue
            out[kind][0] += cycles(a, group, banks)
            out[kind][1] += -(-len(a) // group)

    # staging: position n of the segment goes to skew(bitrev(n))
    nvl = max(1, R // vs)
    for c in range(nvl):
        for s in range(vs):
            def st(l, c=c, s=s):
                tm, t = divmod(l, team)
                v = t + team * c
                if v * vs >= F:
                    return None
                return tm * pitch + pmap(bitrev(v * vs + s, L))
            add("stage", st, 16, 16)
    j = 0
    for p in range(passes):
        rs = r0 if p == 0 else r
        for i in range(R):
            def rd(l, i=i, j=j, rs=rs):
                tm, t = divmod(l, team)
                return tm * pitch + pmap(point_index(t, i, R, j, rs)[0])
            add("read", rd, 32, 32)
            if p + 1 < passes:
                add("write", rd, 16, 16)
        for q in range(rs):
            for i in range(R):
                if i & (1 << q):
                    continue
                def tw(l, i=i, j=j, rs=rs, q=q):
                    t = l % team
                    _, v, ii = point_index(t, i, R, j, rs)
                    k = ((ii & ((1 << q) - 1)) << j) | (v & ((1 << j) - 1))
                    return tmap(k << (L - 1 - (j + q)))
                add("twiddle", tw, 32, 32)
        j += rs
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="fold", choices=sorted(MAPS))
    ap.add_argument("--twiddle-map", default=None, choices=sorted(MAPS))
    ap.add_argument("--vec", type=int, default=1, help="samples of one staging load (1: the general path)")
    a = ap.parse_args()
    pmap, tmap = MAPS[a.map], MAPS[a.twiddle_map or a.map]
    print(f"points: {a.map}, twiddles: {a.twiddle_map or a.map}, vec {a.vec}; LDS cycles of one segment per workgroup / conflict-free cycles")
    for F in (64, 128, 256, 512, 1024, 2048, 4096):
        m = model(F, pmap, tmap, a.vec)
        tot = sum(v[0] for v in m.values()), sum(v[1] for v in m.values())
        print(f"F {F:5d}: " + "  ".join(f"{k} {v[0]:5d}/{v[1]:5d}" for k, v in m.items()) + f"  total x{tot[0] / tot[1]:.2f}")
