"""The hash of brx_hash_batch (include/brx.h) on the CPU, on Python integers, twice: hash_direct is the definition word for word (the
sum with pow(K, U - u, p)); hash_chunked cuts the record into pieces of whole words, takes each by Horner's rule and joins them with
the composition law S(A || B) = S(A) * K^(U_B) + S(B).  tests/test_hash_abi.py holds the two to each other and to the contract's check
values; tests/test_gpu_hash.py and tools/gpu_hash_rate.py take every expected value from here.  Which bytes a record is comes from
tests/take_oracle.py: the two passes share the rule."""
import struct

import numpy as np

import take_oracle

P = (1 << 61) - 1
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(x):
    """the splitmix64 finalizer: a bijection on 64-bit words, mix(0) = 0"""
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ x >> 31


def key(seed):
    """K(seed), in [2, p - 2]"""
    return 2 + mix((seed + GOLDEN) & M64) % (P - 3)


def words(r):
    """the little-endian 32-bit words of r, bytes at or behind len(r) taken as 0"""
    r = bytes(r)
    U = (len(r) + 3) // 4
    return struct.unpack("<%dI" % U, r + bytes(4 * U - len(r)))


def h_direct(r, seed):
    """h(r) = (L + sum c_u K^(U - u)) mod p, term by term"""
    K, c = key(seed), words(r)
    U = len(c)
    return (len(r) + sum(cu * pow(K, U - u, P) for u, cu in enumerate(c))) % P


def hash_direct(r, seed):
    return mix(h_direct(r, seed))


def S_horner(c, K):
    """S of the words c: sum c_u K^(U - u) = (..((c_0) K + c_1) K .. + c_(U-1)) K"""
    acc = 0
    for cu in c:
        acc = (acc + cu) * K % P
    return acc


def S_chunked(r, K, chunk_words):
    c = words(r)
    acc = 0
    for a in range(0, len(c), chunk_words):
        piece = c[a:a + chunk_words]
        acc = (acc * pow(K, len(piece), P) + S_horner(piece, K)) % P
    return acc


def hash_chunked(r, seed, chunk_words=4):
    return mix((len(r) + S_chunked(r, key(seed), chunk_words)) % P)


def as_i64(h):
    """the 64-bit pattern as the int64 that a device tensor holds"""
    return h - (1 << 64) if h >> 63 else h


def hash_records(arena, src, L, seed):
    """int64 array: the hash of arena[src[j] .. src[j] + L[j]) for every j (equal records are hashed once)"""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    K, memo = key(seed), {}
    out = np.empty(len(src), dtype=np.int64)
    for j, (a, ln) in enumerate(zip(src, L)):
        r = arena[int(a):int(a) + int(ln)].tobytes()
        v = memo.get(r)
        if v is None:
            v = memo[r] = as_i64(mix((len(r) + S_horner(words(r), K)) % P))
        out[j] = v
    return out


def hash_take(arena, off, length, count, pos_off, pos, n_pos, D, flags, seed, si=None, sk=None, m=None):
    """(hash, L) of a whole call, the selection as for take_oracle.take_vec"""
    src, L = take_oracle.take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags, si, sk, m)
    return hash_records(arena, src, L, seed), np.asarray(L, dtype=np.int64)


# the contract's check values: seed -> (K, {record: hash})
R256 = bytes(range(256))
CHECK = {
    0: (0x220a8397b1dcdcd, {b"a": 0xba350051cabf3ed3, b"a\0": 0xbb6016563a245eba, b"abcd": 0xada6cd48c13c1c39, b"abcde": 0xf35fc97551548103,
                            b"hello, world\n": 0x0be5baf8a63cf33d, R256: 0x5bb278495e403ce2}),
    1: (0x110a2dec89025cd3, {b"a": 0x4d210b0efb807995, b"a\0": 0x201b4b401d4bfd95, b"abcd": 0x48e414395e8656fd, b"abcde": 0x78061f9a959b2150,
                             b"hello, world\n": 0x6879e40593ee90c8, R256: 0x4540b5719777dafd}),
    M64: (0x4d971771b652c3e, {b"a": 0xc98a66ada32c9c2d, b"abcd": 0x5032cab1b617812b, b"hello, world\n": 0x4e8c2d5bfbc9d732,
                              R256: 0x0bc6190075701881}),
}
CHECK_PRE_MIX = {b"a": 0x0e5fbdc7a64afab4, b"abcd": 0x1117ffd3c0071df7}  # h at seed 0
