"""The rule of brx_take_batch (include/brx.h) on the CPU, twice: the *_serial functions are the contract word for word, one entry and
one byte at a time; the *_vec functions are the same in numpy, fast enough for the GPU tests' batches.  tests/test_take_abi.py holds
the second to the first on random inputs; tests/test_gpu_take.py and tools/gpu_take_rate.py take every expected value from here.

Tables are sequences / int64 arrays as the device holds them: off, length, count, pos_off (n entries), pos (any length; entries are
read as unsigned 64-bit), n_pos <= len(pos).  A selection is two arrays (stream, record) of m entries."""
import numpy as np

NO_DELIM = 1
TRIM_CR = 2
CR = 13


def entries_all_serial(count, pos_off, m):
    """All-records mode: entry j is record j - (pos_off[i] + i) of stream i, the last stream with pos_off[i] + i <= j."""
    n = len(count)
    si, sk = [], []
    for j in range(m):
        i = None
        for t in range(n):
            if int(pos_off[t]) + t <= j:
                i = t
        if i is None:
            si.append(n), sk.append(0)
        else:
            si.append(i), sk.append(j - (int(pos_off[i]) + i))
    return si, sk


def entries_all_vec(count, pos_off, m):
    n = len(count)
    keys = np.asarray(pos_off, dtype=np.int64) + np.arange(n, dtype=np.int64)
    j = np.arange(m, dtype=np.int64)
    i = np.searchsorted(keys, j, side="right") - 1
    none = i < 0
    i = np.where(none, 0, i)
    return np.where(none, n, i), np.where(none, 0, j - keys[i])


def _u64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF


def record_serial(arena, off, length, count, pos_off, pos, n_pos, D, flags, i, k):
    """(source offset in the arena, L) of record k of stream i; (0, 0) where the entry selects nothing."""
    i, k = _u64(i), _u64(k)
    if i >= len(length) or k > int(count[i]):
        return 0, 0
    ln = int(length[i])

    def P(kk):
        idx = int(pos_off[i]) + kk
        if idx >= n_pos:
            return ln
        return min(_u64(pos[idx]), ln)

    start = 0 if k == 0 else min(P(k - 1) + D, ln)
    if k < int(count[i]):
        end = P(k) if flags & NO_DELIM else min(P(k) + D, ln)
    else:
        end = ln
    end = max(end, start)
    if flags & TRIM_CR and end > start and arena[int(off[i]) + end - 1] == CR:
        end -= 1
    return int(off[i]) + start, end - start


def records_serial(arena, off, length, count, pos_off, pos, n_pos, D, flags, si, sk):
    r = [record_serial(arena, off, length, count, pos_off, pos, n_pos, D, flags, i, k) for i, k in zip(si, sk)]
    return [a for a, _ in r], [b for _, b in r]


def records_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags, si, sk):
    arena = np.asarray(arena, dtype=np.uint8)
    off, length, count, pos_off = (np.asarray(a, dtype=np.int64) for a in (off, length, count, pos_off))
    posu = np.asarray(pos, dtype=np.int64).astype(np.uint64) if len(pos) else np.zeros(1, dtype=np.uint64)
    si, sk = np.asarray(si, dtype=np.int64), np.asarray(sk, dtype=np.int64)
    n = len(length)
    if n == 0:
        return np.zeros(len(si), dtype=np.int64), np.zeros(len(si), dtype=np.int64)
    ic = np.where((si >= 0) & (si < n), si, 0)
    valid = (si >= 0) & (si < n) & (sk >= 0) & (sk <= count[ic])
    kc = np.where(valid, sk, 0)
    ln, base = length[ic], pos_off[ic]

    def P(k):
        idx = base + k
        ok = idx < n_pos
        v = posu[np.where(ok, idx, 0)]
        return np.where(ok, np.minimum(v, ln.astype(np.uint64)).astype(np.int64), ln)

    start = np.where(kc > 0, np.minimum(P(np.maximum(kc - 1, 0)) + D, ln), 0)
    e = P(kc)
    if not flags & NO_DELIM:
        e = np.minimum(e + D, ln)
    end = np.maximum(np.where(kc < count[ic], e, ln), start)
    if flags & TRIM_CR:
        last = arena[np.where(end > start, off[ic] + end - 1, 0)] if len(arena) else np.zeros(len(si), dtype=np.uint8)
        end = end - ((end > start) & (last == CR))
    return np.where(valid, off[ic] + start, 0), np.where(valid, end - start, 0)


def fill_serial(arena, src, L, dst_off, total, dst):
    """dst (a bytearray / uint8 array of at least `total` bytes, changed in place and returned): dst[dst_off[j] + t] = arena[src[j] + t]
    for t < min(L[j], room of j); nothing at or beyond total."""
    m = len(src)
    for j in range(m):
        e = int(dst_off[j + 1]) if j + 1 < m else total
        for t in range(int(L[j])):
            d = int(dst_off[j]) + t
            if d >= e or d >= total:
                break
            dst[d] = arena[int(src[j]) + t]
    return dst


def fill_vec(arena, src, L, dst_off, total, dst):
    arena = np.asarray(arena, dtype=np.uint8)
    src, L, dst_off = (np.asarray(a, dtype=np.int64) for a in (src, L, dst_off))
    m = len(src)
    if m == 0:
        return dst
    nxt = np.concatenate([dst_off[1:], np.array([total], dtype=np.int64)])
    cnt = np.maximum(np.minimum(np.minimum(L, nxt - dst_off), total - dst_off), 0)
    tot = int(cnt.sum())
    if tot == 0:
        return dst
    first = np.cumsum(cnt) - cnt
    t = np.arange(tot, dtype=np.int64) - np.repeat(first, cnt)
    dst[np.repeat(dst_off, cnt) + t] = arena[np.repeat(src, cnt) + t]
    return dst


def take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags, si=None, sk=None, m=None):
    """(src, L) of a whole call; si / sk None = all-records mode over m entries (default sum(count) + n)."""
    if si is None:
        if m is None:
            m = int(np.asarray(count, dtype=np.int64).sum()) + len(length)
        si, sk = entries_all_vec(count, pos_off, m)
    return records_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags, si, sk)


def index_positions(arena, off, length, delims):
    """count, pos_off, pos of a plain index at a set of delimiter bytes (what brx_index_batch / brx_index_set_batch with both flags
    report), for building inputs without a device."""
    arena = np.asarray(arena, dtype=np.uint8)
    hit = np.isin(arena, np.frombuffer(bytes(delims), dtype=np.uint8))
    count, pos = [], []
    for o, ln in zip(off, length):
        p = np.flatnonzero(hit[int(o):int(o) + int(ln)])
        count.append(len(p)), pos.append(p)
    count = np.asarray(count, dtype=np.int64)
    pos = np.concatenate(pos).astype(np.int64) if pos else np.zeros(0, dtype=np.int64)
    return count, np.cumsum(count) - count, pos
