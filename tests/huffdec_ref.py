"""Plain-Python restatement of the device Huffman decoder's chain (csrc/jpeg_huffdec.hip): states, rounds, the write
pass's re-check, the DC prefix and max_l1.  It takes the file's scan plan (segment ranges, tables in lookup form) from
jpeg.scan_plan and decodes the bits itself.  `subseq` = stream bytes per subsequence, `group` = subsequences that iterate among
themselves inside one round (the kernel's workgroup; 1 = every exit state travels one subsequence per round)."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
KERNEL_SUBSEQ, KERNEL_GROUP, KERNEL_DEFAULT_ROUNDS = 64, 256, 4       # jpeg_huffdec.hip's SUBSEQ, GROUP, DEFAULT_ROUNDS
OK_RUN, SHORT, BAD = 0, 1, 2


class _Table:
    def __init__(self, t):
        self.fast_len, self.fast_val = list(t.fast_len), list(t.fast_val)
        self.maxcode, self.mincode, self.valptr, self.vals = list(t.maxcode), list(t.mincode), list(t.valptr), list(t.vals)


class Chain:
    """One file's chain.  State = (byte, bit, k, blk): the byte that holds the next bit, bits of it used, zigzag index (0 = at
    DC), block inside the MCU; None = no valid exit (the run met an error or the segment's end)."""

    def __init__(self, data, desc, plan, subseq=KERNEL_SUBSEQ, group=KERNEL_GROUP):
        self.f, self.d, self.subseq, self.group = bytes(data), desc, subseq, group
        self.hsvs = desc.hs * desc.vs
        self.bpm = self.hsvs + (2 if desc.components == 3 else 0)
        self.mcus = desc.mcus_x * desc.mcus_y
        self.interval = plan.restart_interval or self.mcus
        comp = [0 if b < self.hsvs else b - self.hsvs + 1 for b in range(self.bpm)]
        dc, ac = [_Table(plan.dc[0]), _Table(plan.dc[1])], [_Table(plan.ac[0]), _Table(plan.ac[1])]
        self.dct = [dc[plan.dc_sel[c]] for c in comp]
        self.act = [ac[plan.ac_sel[c]] for c in comp]
        self.comp = comp
        self.lanes = []                  # (segment index, segment begin, segment end, first?, last?, subsequence begin, stop)
        for s in range(plan.segments):
            b, e = plan.seg[s].begin, plan.seg[s].end
            cnt = max(1, -(-(e - b) // subseq))
            for j in range(cnt):
                o = b + j * subseq
                self.lanes.append((s, b, e, j == 0, j == cnt - 1, o, e if j == cnt - 1 else o + subseq))
        n = len(self.lanes)
        self.E, self.X, self.N = [None] * n, [None] * n, [0] * n
        self.rounds = 0

    # ---- one run: decode from `state` until the position reaches `stop` (or, writing, until block g_end is complete)
    def run(self, state, seg_end, stop, write=None, g=0, g_end=0):
        f = self.f
        pos, bit, k, blk = state
        nb = 0
        rc = OK_RUN
        while pos < stop:
            if write is not None and g + nb >= g_end:
                break
            nx, w, q = [], 0, pos
            for _ in range(5):
                nx.append(q)
                c = f[q] if q < seg_end else 0
                w = (w << 8) | c
                q += 2 if c == 0xFF else 1
            acc = (w << (24 + bit)) & 0xFFFFFFFFFFFFFFFF
            T = self.dct[blk] if k == 0 else self.act[blk]
            idx = acc >> 55
            l, sym = T.fast_len[idx], T.fast_val[idx]
            if l == 0:
                code16 = acc >> 48
                for ln in range(10, 17):
                    c = code16 >> (16 - ln)
                    if c <= T.maxcode[ln]:
                        sym, l = T.vals[(T.valptr[ln] + c - T.mincode[ln]) & 255], ln
                        break
                if l == 0:
                    rc = BAD
                    break
            s, r = (sym, 0) if k == 0 else (sym & 15, sym >> 4)
            if k == 0 and sym > 15:
                rc = BAD
                break
            t = bit + l + s
            if nx[(t - 1) >> 3] >= seg_end:
                rc = SHORT
                break
            val = 0
            if s:
                v = ((acc << l) & 0xFFFFFFFFFFFFFFFF) >> (64 - s)
                val = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
            end_block = False
            if k == 0:
                if write is not None:
                    write(g + nb, 0, val)
                k = 1
            elif s == 0:
                if r == 15:
                    k += 16
                    end_block = k >= 64
                else:
                    end_block = True
            else:
                k += r
                if k > 63:
                    rc = BAD
                    break
                if write is not None:
                    write(g + nb, ZIGZAG[k], val)
                k += 1
                end_block = k == 64
            pos, bit = nx[t >> 3], t & 7
            if end_block:
                k, nb, blk = 0, nb + 1, (blk + 1) % self.bpm
        return rc, (pos, bit, k, blk), nb

    def _decode(self, i):
        s, b, e, first, last, o, stop = self.lanes[i]
        rc, st, nb = self.run(self.E[i], e, stop)
        return (st if rc == OK_RUN else None), nb

    def round(self):
        """e_i <- x_(i-1), re-decode what changed; the lanes of a group iterate until nothing changes"""
        r, f = self.rounds, self.f
        xprev = list(self.X)
        for g0 in range(0, len(self.lanes), self.group):
            ids = range(g0, min(g0 + self.group, len(self.lanes)))
            need = set()
            for i in ids:
                s, b, e, first, last, o, stop = self.lanes[i]
                if first:
                    self.E[i] = (b, 0, 0, 0)
                elif r == 0:
                    p = o + 1 if (f[o] == 0 and f[o - 1] == 0xFF) else o
                    self.E[i] = (p, 0, 0, 0)
                if r == 0:
                    need.add(i)
                    self.X[i] = None
            for _ in range(self.group + 1):
                sx = {i: self.X[i] for i in ids}
                for i in ids:
                    if self.lanes[i][3]:
                        continue
                    left = sx[i - 1] if i > g0 else (xprev[i - 1] if r else None)
                    if left is not None and left != self.E[i]:
                        self.E[i] = left
                        need.add(i)
                if not need:
                    break
                for i in need:
                    self.X[i], self.N[i] = self._decode(i)
                need = set()
        self.rounds += 1

    def certify(self, coef=None):
        """The write pass: decode from e_i at the block the prefix sum names, compare every exit with e_(i+1), require every segment
        to complete exactly its blocks inside its last byte.  coef: int16 array to store into (DC differences), or None."""
        P, acc = [], 0
        for v in self.N:
            P.append(acc)
            acc += v
        first_of = {}
        for i, ln in enumerate(self.lanes):
            first_of.setdefault(ln[0], i)
        d = self.d
        total = self.mcus * self.bpm

        def write(g, z, val):
            assert 0 <= g < total
            mcu, b = divmod(g, self.bpm)
            c = self.comp[b]
            h, v = (d.hs, d.vs) if c == 0 else (1, 1)
            by, bx = divmod(b if c == 0 else 0, h)
            y, x = divmod(mcu, d.mcus_x)
            coef[d.coef_off[c] + ((y * v + by) * d.mcus_x * h + x * h + bx) * 64 + z] = np.int16(val)

        for i, (s, b, e, first, last, o, stop) in enumerate(self.lanes):
            if self.E[i] is None:
                return False
            base = P[i] - P[first_of[s]]
            g0 = s * self.interval * self.bpm + base
            g_end = min((s + 1) * self.interval, self.mcus) * self.bpm
            if g0 > g_end or g0 % self.bpm != self.E[i][3]:
                return False
            rc, st, nb = self.run(self.E[i], e, stop, write if coef is not None else (lambda *a: None), g0, g_end)
            if rc != OK_RUN:
                return False
            pos, bit, k, blk = st
            if not last:
                if not (pos >= stop and nb == self.N[i] and st == self.E[i + 1]):
                    return False
            else:
                if g0 + nb != g_end or k != 0 or blk != 0:
                    return False
                if bit == 0:
                    if pos != e:
                        return False
                elif not (pos < e and pos + (2 if self.f[pos] == 0xFF else 1) == e):
                    return False
        return True


def rounds_needed(data, desc, plan, subseq=KERNEL_SUBSEQ, group=KERNEL_GROUP, limit=64):
    """the smallest number of rounds after which the write pass's check holds (None: not within `limit`)"""
    ch = Chain(data, desc, plan, subseq, group)
    for r in range(1, limit + 1):
        ch.round()
        if ch.certify():
            return r
    return None


def decode(data, desc, plan, subseq=KERNEL_SUBSEQ, group=KERNEL_GROUP, max_rounds=KERNEL_DEFAULT_ROUNDS):
    """(ok, int16 coefficients in entropy_decode's layout, max_l1): ok False = the chain's check failed (SSD_JPEG_TO_HOST)"""
    ch = Chain(data, desc, plan, subseq, group)
    for _ in range(max_rounds):
        ch.round()
    d = desc
    mcus, hsvs = ch.mcus, ch.hsvs
    nblocks = mcus * ch.bpm
    coef = np.zeros(nblocks * 64, np.int16)
    if not ch.certify(coef):
        return False, None, 0
    blocks = coef.reshape(nblocks, 64)
    # DC: per component in scan order, the sum restarts where a segment starts; Python integers do not wrap
    for c in range(d.components):
        h, v = (d.hs, d.vs) if c == 0 else (1, 1)
        base = d.coef_off[c] // 64
        pred = 0
        for mcu in range(mcus):
            if mcu % ch.interval == 0:
                pred = 0
            y, x = divmod(mcu, d.mcus_x)
            for by in range(v):
                for bx in range(h):
                    bi = base + (y * v + by) * d.mcus_x * h + x * h + bx
                    pred += int(blocks[bi, 0])
                    if not -32768 <= pred <= 32767:
                        return False, None, 0
                    blocks[bi, 0] = pred
    max_l1 = 0
    for c in range(d.components):
        q = np.array(d.qt[c], np.int64)
        lo = d.coef_off[c] // 64
        hi = d.coef_off[c + 1] // 64 if c + 1 < d.components else nblocks
        if hi > lo:
            max_l1 = max(max_l1, int((np.abs(blocks[lo:hi].astype(np.int64)) * q).sum(1).max()))
    return True, coef, min(max_l1, 0x7fffffff)
