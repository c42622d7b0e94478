"""The cases of tests/test_sumthreshold_kernels_gpu.py, their host reference, and what that module takes for granted,
checked without a GPU.

reference_lines / reference_line restate flagging.py:610-681 (_sum_threshold1d with _convolve_flags) in numpy float64 for
lines whose first threshold is handed in: per chunk the padded slice, per window the clamp against the flags of the
windows before it, the sequential prefix sum, (cum[k + w] - cum[k]) * f64(f32(1 / w)) > thr for both signs, the dilation
over w, and the chunk's interior written out.  Where no chunk covers a position the SENTINEL stays.

CASES is the table both modules run: shapes, window lists, chunk layouts, rho, and a kind per column (KINDS_BY_RHO).
The tests below hold the reference to the oracle, bit for bit, on every column whose MAD is the median of its unflagged
samples, and check on the reference alone that the cases are not vacuous:

  mixed kinds    the columns of a kind noise / bumps / clamp / dense / nonfinite of a case hold flagged and clean samples
  every window   in the bumps columns of a case each distinct window flags a sample that stays clean without that window
                 (cases with at least two bumps columns per window: a column holds one run)
  chunk edges    at every edge between two chunks some bumps column of the case differs, within reach of the edge,
                 from the reference that pads no chunk
  clamps fire    in the clamp and dense columns every window after the first clamps; in clamp_opp a clamp that ignores
                 the sign of the flag changes the result
  ties           tie columns are clean, their twins flag exactly the run

A condition over "a case" is taken over the columns of that kind in all images of the case: one column of a line of
eight samples cannot hold a run of every window in both signs.
"""
import math

import numpy as np
import pytest

SENTINEL = 7
MAD_NORMAL = 1.4826
NSIGMA = 4.5
W1248 = (1, 2, 4, 8)

# the kinds a case deals its columns, by the rho of the case: exact ties need rho = 2 (tf = w) or rho = 1, a sample of
# the other sign under an earlier window's flag needs a second window whose threshold is below half the first (rho > 2)
KINDS_BY_RHO = {
    1.3: ("bumps", "noise", "clamp", "dense", "zero_mad", "nan_mad", "nonfinite", "extremes"),
    2.0: ("tie", "twin", "noise"),
    1.0: ("tie", "twin", "noise"),
    3.0: ("clamp_opp", "noise"),
}
FROM_FLAGS = ("bumps", "noise", "clamp", "dense", "nonfinite", "extremes", "clamp_opp")    # MAD = median of the unflagged
MIXED = ("noise", "bumps", "clamp", "dense", "nonfinite")


def thr0_of(mad, nsigma=NSIGMA):
    """The first threshold as the kernels form it: f32(f64(mad) * (nsigma * 1.4826)), infinite for a NaN MAD."""
    mad = np.asarray(mad, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(mad), np.float32(np.inf), (mad * (nsigma * MAD_NORMAL)).astype(np.float32))


def tf_of(rho, w):
    return math.pow(rho, math.log2(w))


def reference_lines(x, thr0, windows, rho, chunk_ends, pad_maxw=None, two_sided=False):
    """x (L, C) float32, thr0 (C, G) float32.  Returns (flags (L, C) uint8 with SENTINEL outside the chunks,
    clamped (n_windows, C): how many samples each window clamped).  pad_maxw: the window the padding is sized by
    (default max(windows)); two_sided: the clamp ignores which sign flagged the sample."""
    x = np.asarray(x, np.float32)
    L, C = x.shape
    thr0 = np.asarray(thr0, np.float32).reshape(C, -1)
    out = np.full((L, C), SENTINEL, np.uint8)
    nclamp = np.zeros((len(windows), C), np.int64)
    maxw = max(windows) if pad_maxw is None else pad_maxw
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(chunk_ends) - 1):
            c0, c1 = int(chunk_ends[g]), int(chunk_ends[g + 1])
            if c1 <= c0:
                continue
            p0, p1 = max(c0 - maxw + 1, 0), min(c1 + maxw - 1, L)
            Lp = p1 - p0
            xd = x[p0:p1].astype(np.float64)
            pos = np.zeros((Lp, C), bool)
            neg = np.zeros((Lp, C), bool)
            idx = np.arange(Lp)
            for j, w in enumerate(windows):
                thr = thr0[:, g].astype(np.float64) / tf_of(rho, w)
                fp, fn = (pos | neg, pos | neg) if two_sided else (pos, neg)
                cp = fp & (xd > thr)
                cn = ~cp & fn & (xd < -thr)
                cl = np.where(cp, thr, np.where(cn, -thr, xd))
                nclamp[j] += cp.sum(0) + cn.sum(0)
                cum = np.concatenate([np.zeros((1, C)), np.cumsum(cl, axis=0)])      # (sequential along the line)
                M = Lp + 1 - w
                if M <= 0:
                    continue
                S = cum[w:] - cum[:-w]
                scale = np.float64(np.float32(1.0 / w))
                lo, hi = np.clip(idx - w + 1, 0, M), np.clip(idx + 1, 0, M)
                for hits, of in ((S * scale > thr, pos), (S * (-scale) > thr, neg)):
                    hc = np.concatenate([np.zeros((1, C), np.int64), np.cumsum(hits, axis=0)])
                    of |= hc[hi] != hc[lo]
            out[c0:c1] = (pos | neg)[c0 - p0:c1 - p0]
    return out, nclamp


def reference_line(x, thr0_per_chunk, windows, rho, chunk_ends):
    out, nclamp = reference_lines(np.asarray(x, np.float32).reshape(-1, 1), np.asarray(thr0_per_chunk).reshape(1, -1), windows, rho, chunk_ends)
    return out[:, 0], nclamp[:, 0]


# ---- the case table ----

def _case(L, C, windows, ends, rho=1.3, variants=(1, 2, 3, 4), n_win=2, refused=(), nsigma=NSIGMA):
    return dict(L=L, C=C, windows=tuple(windows), ends=[min(int(e), L) for e in ends], rho=rho, variants=tuple(variants), n_win=n_win,
                refused=tuple(refused), nsigma=float(nsigma))


LAYOUTS_96 = {"one": [0, 96], "ones_first": [0, 1, 2, 96], "one_last": [0, 95, 96], "halves": [0, 48, 96], "ones_mid": [0, 7, 8, 9, 96],
              "inset": [3, 93], "empties": [0, 0, 40, 40, 96], "uneven": [0, 17, 33, 64, 96], "fours": list(range(0, 97, 4))}
LAYOUTS_200 = {"halves": [0, 100, 200], "interior": [0, 37, 163, 200]}
LAYOUTS_300 = {"one": [0, 300], "thirds": [0, 100, 200, 300], "ones": [0, 1, 299, 300], "short": [0, 20, 40, 300]}
COLUMN_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320)
WINDOW_LISTS = ((7,), (15, 16, 17), (3, 5, 16, 17, 40), (32, 48, 64, 128), (1, 2, 4, 8, 16, 32, 64, 128), (8, 2, 5), (2, 2, 4))
NINE_WINDOWS = (1, 2, 3, 4, 6, 8, 12, 16, 24)             # one more than the stage pipeline takes


def _pow2(windows):
    return all(w & (w - 1) == 0 for w in windows)


def _build_cases():
    cases = {}
    for rho in KINDS_BY_RHO:
        for L in range(8, 97):
            cases["sweep[L=%d, C=64, rho=%g]" % (L, rho)] = _case(L, 64, W1248, [0, L], rho, (1, 2, 3, 4, 5))
            cases["sweep[L=%d, C=70, rho=%g]" % (L, rho)] = _case(L, 70, W1248, [0, L], rho)
        for name, ends in LAYOUTS_96.items():
            for L in range(89, 97) if rho == 1.3 else (96,):
                cases["layout[%s, L=%d, rho=%g]" % (name, L, rho)] = _case(L, 130, W1248, ends, rho)
        for name, ends in LAYOUTS_200.items():
            cases["layout[%s, L=200, rho=%g]" % (name, rho)] = _case(200, 130, W1248, ends, rho)
    for C in COLUMN_COUNTS:
        for n_win in (1, 3):
            cases["columns[C=%d, n_win=%d]" % (C, n_win)] = _case(64, C, W1248, [0, 64], 1.3, (1, 2, 3, 4, 5) if C % 64 == 0 else (1, 2, 3, 4), n_win)
    for C in (1, 2, 3):                                    # the spectrum pass: one image, a column per window, chunks
        cases["columns[C=%d, n_win=1, chunks]" % C] = _case(64, C, W1248, [0, 23, 64], 1.3, (1, 2, 3, 4), 1)
    for wl in WINDOW_LISTS:
        tag = ",".join(map(str, wl))
        for L in (max(wl), max(wl) + 1):
            # (a run of the widest window buries the line's MAD sample: nsigma puts that sample at the run's level)
            cases["windows[%s, L=%d]" % (tag, L)] = _case(L, 70, wl, [0, L], 1.3, (1, 4), nsigma=tf_of(1.3, max(wl)) / MAD_NORMAL)
        for name, ends in LAYOUTS_300.items():
            cases["windows[%s, L=300, %s]" % (tag, name)] = _case(300, 70, wl, ends, 1.3, (1, 4))
        if _pow2(wl):
            for rho in (2.0, 1.0):
                cases["windows[%s, L=300, thirds, rho=%g]" % (tag, rho)] = _case(300, 70, wl, LAYOUTS_300["thirds"], rho, (1, 4))
    cases["windows[nine, L=300]"] = _case(300, 70, NINE_WINDOWS, LAYOUTS_300["thirds"], 1.3, (1, 4), refused=(4,))
    return cases


CASES = _build_cases()


def accepts(case, variant):
    """Whether the hook documents `variant` as supported for the case."""
    G = len(case["ends"]) - 1
    if variant in (2, 3):
        return case["windows"] == W1248
    if variant == 4:
        return len(case["windows"]) <= 8
    if variant == 5:
        return case["windows"] == W1248 and case["C"] % 64 == 0 and G == 1
    return variant == 1


def comparisons_per_variant():
    """{variant: calls compared with the reference} the table implies."""
    out = {}
    for case in CASES.values():
        for v in case["variants"]:
            if v not in case["refused"]:
                assert accepts(case, v)
                out[v] = out.get(v, 0) + 1
    return out


def kinds_of(case):
    """(n_win, C) kind names and the running number of each column within its kind."""
    names = KINDS_BY_RHO[case["rho"]]
    if case["rho"] == 1.3 and case["C"] >= 4 and len(case["ends"]) > 2:
        # chunked cases: every other column is a bump, one per placement
        names = tuple(n for other in names[1:] for n in ("bumps", other))
    if not _pow2(case["windows"]):
        names = tuple(n for n in names if n not in ("tie", "twin"))
    if case["windows"][:3] != (1, 2, 4):
        names = tuple(n for n in names if n != "clamp_opp")
    kinds = np.empty((case["n_win"], case["C"]), object)
    number = np.zeros((case["n_win"], case["C"]), np.int64)
    seen = {}
    for i in range(case["n_win"]):
        for c in range(case["C"]):
            k = names[(c + i) % len(names)]
            kinds[i, c] = k
            number[i, c] = seen.get(k, 0)
            seen[k] = number[i, c] + 1
    return kinds, number


def _chunks(ends):
    return [(g, ends[g], ends[g + 1]) for g in range(len(ends) - 1) if ends[g + 1] > ends[g]]


def edges_of(ends):
    """(edge, left chunk, right chunk) where two chunks with samples meet."""
    ch = _chunks(ends)
    return [(a[2], a[0], b[0]) for a, b in zip(ch, ch[1:]) if a[2] == b[1]]


def placements(case, w):
    """(start, owner chunk) of the runs of `w` samples a bumps column may hold: the line start and end, astride every chunk
    edge (owned by either side), and the first and last positions of every chunk's padded line."""
    L, ends, maxw = case["L"], case["ends"], max(case["windows"])
    ch = _chunks(ends)
    out = []
    if not ch:
        return out
    out.append((0, ch[0][0]))
    out.append((L - w, ch[-1][0]))
    for e, ga, gb in edges_of(ends):
        out += [(e - max(w // 2, 1), ga), (e - w // 2, gb)]
    out += [(ch[0][1], ch[0][0]), (ch[-1][2] - w, ch[-1][0])]          # the first and last samples any chunk covers
    for g, c0, c1 in ch:
        out += [(max(c0 - maxw + 1, 0), g), (min(c1 + maxw - 1, L) - w, g)]
    seen, uniq = set(), []
    for s, g in out:
        c0, c1 = ends[g], ends[g + 1]
        inside = s >= max(c0 - maxw + 1, 0) and s + w <= min(c1 + maxw - 1, L)
        if 0 <= s and s + w <= L and inside and (s, g) not in seen:
            seen.add((s, g))
            uniq.append((s, g))
    return uniq


def bump_combos(case):
    """(start, owner, w, sign) in the order the bumps columns take them: the placements first, the window rotating."""
    key = (case["L"], tuple(case["ends"]), case["windows"])
    if key not in _COMBOS:
        wl = sorted(set(case["windows"]))
        pls = {w: placements(case, w) for w in wl}
        n = max(len(pl) for pl in pls.values())
        out = []
        for r in range(len(wl)):
            for p in range(n):
                w = wl[(p + r) % len(wl)]
                if p < len(pls[w]):
                    out.append(pls[w][p] + (w, 1.0 if (p + r) % 2 == 0 else -1.0))
        _COMBOS[key] = out
    return _COMBOS[key]


_COMBOS = {}


def _bump_level(case, w):
    """The run's level relative to thr_w: above it, below what a narrower window needs, and low enough that no wider
    window reaches its threshold on the run alone; 1.05 where those leave room."""
    rho = case["rho"]
    rel = lambda v: tf_of(rho, w) / tf_of(rho, v)           # thr_v / thr_w
    upper = [rel(v) for v in case["windows"] if v < w] + [rel(v) * v / w for v in case["windows"] if v > w]
    room = min(upper) - 1.0 if upper else 1.0
    return min(1.05, 1.0 + 0.4 * room), 1.0 + 0.7 * room


class _Column:
    """One line under construction: samples, input flags (everything flagged that is not a MAD carrier), MADs."""

    def __init__(self, case, rs, base):
        self.case, self.rs = case, rs
        self.L, self.ends = case["L"], case["ends"]
        self.G = len(self.ends) - 1
        self.x = (rs.standard_normal(self.L) * 1e-3 * base).astype(np.float32)
        self.flags = np.ones(self.L, bool)
        self.taken = np.zeros(self.L, bool)
        self.mad = np.full(self.G, np.nan)
        # the MAD each chunk is going to have: one unflagged sample of this size
        self.m = {g: np.float32(base * (1.0 + 0.1 * rs.uniform())) for g, _, _ in _chunks(self.ends)}

    def thr0(self, g):
        return float(np.float32(np.float64(self.m[g]) * (self.case["nsigma"] * MAD_NORMAL)))

    def thr(self, g, w):
        return self.thr0(g) / tf_of(self.case["rho"], w)

    def put(self, p, v):
        if 0 <= p < self.L and not self.taken[p]:
            self.x[p] = np.float32(v)
            self.taken[p] = True
            return True
        return False

    def carriers(self, reach=8, done=()):
        """Gives every chunk its unflagged sample, away from what was put before where the chunk has room; a chunk that
        is full takes one of the samples that fill it."""
        for g, c0, c1 in _chunks(self.ends):
            if g in done:
                continue
            free = c0 + np.flatnonzero(~self.taken[c0:c1])
            if free.size:
                near = np.convolve(self.taken, np.ones(2 * reach + 1), "same")[free] > 0
                pick = free[~near] if (~near).any() else free
                p = int(pick[int(self.rs.randint(len(pick)))])
                self.x[p] = self.m[g] * (1.0 if self.rs.uniform() < 0.5 else -1.0)
            else:
                p = c0 + int(self.rs.randint(c1 - c0))
            self.taken[p] = True
            self.flags[p] = False
            self.mad[g] = abs(float(self.x[p]))


def _owner(col, k):
    ch = [c for c in _chunks(col.ends) if c[2] - c[1] >= 2] or _chunks(col.ends)
    return ch[k % len(ch)] if ch else None


def _column(case, kind, k, rs):
    """(x, flags or None, mad (G,), info) of column number k of its kind."""
    L, ends, windows, rho = case["L"], case["ends"], case["windows"], case["rho"]
    G, maxw = len(ends) - 1, max(windows)
    info = {}
    if kind == "noise":
        x = (rs.standard_normal(L) * 2.0).astype(np.float32)
        x[L // 3] += 30.0
        x[int(rs.randint(L))] -= 25.0
        x[-1] += 40.0 * (k % 2)
        x[0] -= 40.0 * (k // 2 % 2)
        if min(windows) > 8:
            x[L // 3:L // 3 + 40] += 6.0                     # a broad bump for lists without a narrow window
        flags = rs.uniform(size=L) < 0.1
        mad = np.full(G, np.nan)
        for g, c0, c1 in _chunks(ends):
            keep = np.flatnonzero(~flags[c0:c1])
            if keep.size and keep.size % 2 == 0:             # an odd count: the median is a sample
                flags[c0 + keep[0]] = True
                keep = keep[1:]
            if keep.size:
                mad[g] = np.sort(np.abs(x[c0:c1][keep]))[keep.size // 2]
        return x, flags, mad, info
    if kind in ("zero_mad", "nan_mad"):
        x = (rs.standard_normal(L) * 2.0).astype(np.float32)
        x[rs.uniform(size=L) < 0.3] = 0.0
        x[rs.uniform(size=L) < 0.05] = -0.0
        x[L // 2] = 50.0
        other = 0.7 if kind == "zero_mad" else 0.3
        mad = np.array([(0.0 if kind == "zero_mad" else np.nan) if (g + k) % 3 else other for g in range(G)])
        if G == 1:
            mad[:] = 0.0 if kind == "zero_mad" else np.nan
        return x, None, mad, info
    if kind in ("tie", "twin"):
        pw = [w for w in sorted(set(windows))]
        w = pw[k % len(pw)]
        m = 0.5 + 0.25 * (k % 7)
        mad = np.full(G, m)
        t0 = np.float32(thr0_of(m, case["nsigma"]))
        x = np.zeros(L, np.float32)
        s = (k * 7) % (L - w + 1)
        sign = np.float32(1.0 if k // len(pw) % 2 == 0 else -1.0)
        v = np.float32(t0 / np.float32(w)) if rho == 2.0 else t0
        x[s:s + w] = v
        if kind == "twin":
            up = np.nextafter(v, np.float32(np.inf))
            if rho == 2.0:
                x[s + k % w] = up
            else:
                x[s:s + w] = up      # (one raised sample alone would be flagged by window 1, and its clamp restores the tie)
        x *= sign
        info.update(run=(s, s + w), w=w)
        return x, None, mad, info
    base = float(10.0 ** rs.uniform(-2, 2))
    if kind == "extremes":
        base = 1e-38 if k % 2 == 0 else 1e37
    col = _Column(case, rs, base)
    if kind == "bumps":
        combos = bump_combos(case)
        s, g, w, sign = combos[k % len(combos)]
        c0, c1 = ends[g], ends[g + 1]
        level, most = _bump_level(case, w)
        level, most = level * col.thr(g, w), most * col.thr(g, w)
        if w >= L and (k // len(combos)) % 2:
            level *= 0.9          # a run that is the whole line flags all of it: every other one stays just short
        inside = [p for p in range(c0, c1) if not s <= p < s + w]
        amp = level
        if not inside and w > 1:
            # the owner lies inside the run: its MAD sample stays small, the others make up for it
            amp = (level * w - float(col.m[g])) / (w - 1)
            if amp >= most:
                amp = level                                   # no room: the run stays short of its threshold
        for p in range(s, s + w):
            col.put(p, sign * amp)
        done = ()
        if not inside:
            p = c0 + k % (c1 - c0)
            col.x[p] = sign * col.m[g]
            col.flags[p] = False
            col.mad[g] = float(col.m[g])
            done = (g,)
        info.update(run=(s, s + w), w=w, owner=g)
        col.carriers(reach=maxw, done=done)
        return col.x, col.flags, col.mad, info
    own = _owner(col, k)
    if own is None:
        col.carriers()
        return col.x, col.flags, col.mad, info
    g, c0, c1 = own
    t0 = col.thr0(g)
    sign = 1.0 if k % 2 == 0 else -1.0
    s = c0 + (k * 5) % (c1 - c0)
    if kind == "clamp":
        col.put(s, sign * 3.0 * t0 * windows[0])
        for p in range(s - maxw + 1, s + maxw):
            col.put(p, sign * 0.95 * col.thr(g, maxw))
    elif kind == "clamp_opp":
        s = min(s, max(L - 4, 0))
        for p, v in zip(range(s, s + 4), (0.3, 0.98, -0.2, 0.38)):
            col.put(p, sign * v * t0)
    elif kind == "dense":
        n = max(min(maxw + 3 + k % 5, L - 1), 1)
        s = min(s, L - n)
        for p in range(s, s + n):
            col.put(p, sign * 2.0 * t0)
    elif kind == "nonfinite":
        special = (np.inf, -np.inf, np.nan)[k % 3]
        ed = edges_of(ends)
        s = ed[(k // 6) % len(ed)][0] + 2 if ed and (k // 3) % 2 else L // 2
        col.put(min(s, L - 1), special)
        for p in (1, s - 5, s + 5, L - 2):                   # finite outliers before and behind it
            col.put(p, sign * 5.0 * t0)
    elif kind == "extremes":
        col.put(s, sign * 3.0 * t0)
        w = windows[k % len(windows)]
        s2 = (s + 2 * maxw) % max(L - w, 1)
        for p in range(s2, s2 + w):
            col.put(p, -sign * 1.05 * col.thr(g, w))
    col.carriers()
    return col.x, col.flags, col.mad, info


_MADE = {}


def make_case(name):
    """dict(data (n_win, L, C) float32, flags (n_win, L, C) bool, mad (n_win, C, G) float64, kinds, number, info) of a
    case: the same arrays for every caller (kept; do not write to them)."""
    if name in _MADE:
        return _MADE[name]
    case = CASES[name]
    n_win, L, C, G = case["n_win"], case["L"], case["C"], len(case["ends"]) - 1
    kinds, number = kinds_of(case)
    data = np.zeros((n_win, L, C), np.float32)
    flags = np.zeros((n_win, L, C), bool)
    mad = np.zeros((n_win, C, G))
    info = {}
    import zlib
    for i in range(n_win):
        for c in range(C):
            rs = np.random.RandomState(zlib.crc32(("%s/%d/%d" % (name, i, c)).encode()) & 0x7FFFFFFF)
            x, f, m, inf = _column(case, kinds[i, c], int(number[i, c]), rs)
            data[i, :, c] = x
            if f is not None:
                flags[i, :, c] = f
            mad[i, c] = m
            info[i, c] = inf
    made = dict(case=case, data=data, flags=flags, mad=mad, kinds=kinds, number=number, info=info)
    for a in (data, flags, mad):
        a.setflags(write=False)
    _MADE[name] = made
    return made


def reference_of(made, **kw):
    """(flags (n_win, L, C) uint8, clamped (n_windows, n_win, C)) of a made case by reference_lines."""
    if not kw and "ref" in made:
        return made["ref"]
    case = made["case"]
    n_win, L, C = made["data"].shape
    x = np.ascontiguousarray(made["data"].transpose(1, 0, 2)).reshape(L, n_win * C)
    thr0 = thr0_of(made["mad"], case["nsigma"]).reshape(n_win * C, -1)
    out, ncl = reference_lines(x, thr0, case["windows"], case["rho"], case["ends"], **kw)
    ref = np.ascontiguousarray(out.reshape(L, n_win, C).transpose(1, 0, 2)), ncl.reshape(len(case["windows"]), n_win, C)
    if not kw:
        ref[0].setflags(write=False)
        made["ref"] = ref                                   # (computed once, shared, left unchanged)
    return ref


def family(name):
    return name.split("[", 1)[0] + ("" if "rho=" not in name else "/rho=" + name.rsplit("rho=", 1)[1].rstrip("]"))


FAMILIES = sorted({family(n) for n in CASES})


def cases_of(fam):
    return [n for n in CASES if family(n) == fam]


# ---- the tests ----

# the size of the table: cases, and calls compared with the reference per variant
EXPECTED_CASES = 893
EXPECTED_COMPARISONS = {1: 893, 2: 846, 3: 846, 4: 892, 5: 364}

def test_the_table_is_what_the_gpu_module_counts():
    assert len(CASES) == EXPECTED_CASES, len(CASES)
    assert comparisons_per_variant() == EXPECTED_COMPARISONS, comparisons_per_variant()
    assert set(cases_of(FAMILIES[0])) and sum(len(cases_of(f)) for f in FAMILIES) == len(CASES)
    refused = [(n, v) for n, c in CASES.items() for v in c["refused"]]
    assert refused == [("windows[nine, L=300]", 4)]
    for name, case in CASES.items():
        assert max(case["windows"]) <= case["L"], name
        assert all(a <= b for a, b in zip(case["ends"], case["ends"][1:])) and 0 <= case["ends"][0] and case["ends"][-1] <= case["L"], name
        for v in (1, 2, 3, 4, 5):
            # nothing the hook supports is left out, but the panel form of the chunk-layout and window-list families
            if accepts(case, v) and v not in case["variants"]:
                assert v == 5 and case["C"] % 64 == 0, (name, v)



def test_reference_line_is_the_columns_form():
    made = make_case("layout[uneven, L=96, rho=1.3]")
    ref, ncl = reference_of(made)
    case = made["case"]
    for c in range(0, case["C"], 7):
        one, n1 = reference_line(made["data"][1, :, c], thr0_of(made["mad"][1, c], case["nsigma"]), case["windows"], case["rho"], case["ends"])
        assert np.array_equal(one, ref[1, :, c]) and np.array_equal(n1, ncl[:, 1, c])


@pytest.mark.parametrize("fam", FAMILIES)
def test_reference_equals_the_oracle(oracle, fam):
    """Bit for bit on every column whose MAD is the median of its unflagged samples -- which the oracle's own median
    must reproduce -- and the sentinel exactly where no chunk covers."""
    compared = 0
    for name in cases_of(fam):
        made = make_case(name)
        case = made["case"]
        ref, _ = reference_of(made)
        lo, hi = case["ends"][0], case["ends"][-1]
        assert (ref[:, :lo] == SENTINEL).all() and (ref[:, hi:] == SENTINEL).all() and (ref[:, lo:hi] <= 1).all(), name
        for i in range(case["n_win"]):
            cols = np.flatnonzero(np.isin(made["kinds"][i], FROM_FLAGS))
            if not cols.size:
                continue
            x, f = made["data"][i][:, cols], made["flags"][i][:, cols]
            for g, c0, c1 in _chunks(case["ends"]):
                med = oracle.median_abs_axis0(x[c0:c1], f[c0:c1]).reshape(-1).astype(np.float64)
                assert np.array_equal(med, made["mad"][i, cols, g], equal_nan=True), (name, i, g)
            exp = oracle.sum_threshold(np.ascontiguousarray(x.T), np.ascontiguousarray(f.T), 1, np.array(case["windows"]), case["nsigma"],
                                       case["rho"], chunks=np.array(case["ends"])).T
            assert np.array_equal(ref[i, lo:hi][:, cols] != 0, exp[lo:hi]), (name, i, int((ref[i, lo:hi][:, cols] != exp[lo:hi]).sum()))
            compared += cols.size
    assert compared > 0, fam


def _columns(made, kind):
    return [(i, c) for i in range(made["kinds"].shape[0]) for c in range(made["kinds"].shape[1]) if made["kinds"][i, c] == kind]


def _without(made, **kw):
    """The reference of a made case under another window list (`windows`) or reference switch."""
    windows = kw.pop("windows", None)
    if windows is not None:
        made = dict(made, case=dict(made["case"], windows=tuple(windows)))
    return reference_of(made, **kw)[0]


@pytest.mark.parametrize("fam", FAMILIES)
def test_cases_are_not_vacuous(fam):
    for name in cases_of(fam):
        made = make_case(name)
        case = made["case"]
        ends, windows, maxw = case["ends"], case["windows"], max(case["windows"])
        lo, hi = ends[0], ends[-1]
        ref, ncl = reference_of(made)
        cov = ref[:, lo:hi]
        for kind in MIXED:
            cols = _columns(made, kind)
            if cols:
                frac = np.mean([cov[i, :, c].mean() for i, c in cols])
                # (a line shorter than two of its narrowest windows: the hits of a clamp or dense column, which always hits,
                # dilate over all of it; a line with no room for a run longer than every window: the dense run is the line)
                whole = (case["L"] < 2 * min(windows) and kind in ("clamp", "dense")) or (case["L"] <= maxw + 3 and kind == "dense")
                assert 0 < frac and (frac < 1 or whole), (name, kind, frac)
        for kind in ("clamp", "dense"):
            cols = _columns(made, kind)
            if cols:
                per_window = sum(ncl[:, i, c] for i, c in cols)
                assert (per_window[1:] > 0).all(), (name, kind, per_window)
        cols = _columns(made, "clamp_opp")
        if cols:
            two = _without(made, two_sided=True)
            assert any((two[i, :, c] != ref[i, :, c]).any() for i, c in cols), name
        for kind in ("tie", "twin"):
            for i, c in _columns(made, kind):
                run = np.zeros(case["L"], bool)
                s, e = made["info"][i, c]["run"]
                run[s:e] = True
                want = (run & (kind == "twin"))[lo:hi]
                assert np.array_equal(cov[i, :, c] != 0, want), (name, kind, i, c, made["info"][i, c])
        for i, c in _columns(made, "zero_mad") + _columns(made, "nan_mad"):
            x, m = made["data"][i, :, c], made["mad"][i, c]
            for g, c0, c1 in _chunks(ends):
                if m[g] == 0.0 and 1 in windows:
                    assert ((x[c0:c1] != 0) <= (ref[i, c0:c1, c] != 0)).all(), (name, i, c)
                if np.isnan(m[g]):
                    assert not ref[i, c0:c1, c].any(), (name, i, c)
        cols = _columns(made, "bumps")
        if cols:
            for w in sorted(set(windows)):
                rest = [v for v in windows if v != w]
                # (a column holds one run: fewer columns than two per window cannot hold a run of each)
                if not rest or len(cols) < 2 * len(set(windows)):
                    continue
                # (the padding keeps the size the full list gives it)
                less = _without(made, windows=rest, pad_maxw=maxw)
                assert any(((ref[i, lo:hi, c] == 1) & (less[i, lo:hi, c] == 0)).any() for i, c in cols), (name, "window", w)
            if maxw > 1:
                bare = _without(made, pad_maxw=1)
                # (as above: a column holds one run, and every edge needs one owned by either side)
                for e, ga, gb in edges_of(ends) if len(cols) >= 2 * len(edges_of(ends)) else ():
                    a, b = max(ends[ga], e - maxw + 1), min(ends[gb + 1], e + maxw - 1)
                    assert any((ref[i, a:b, c] != bare[i, a:b, c]).any() for i, c in cols), (name, "edge", e)
