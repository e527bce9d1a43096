// decompressor.hpp -- C++ host-side mirror of the reference's only public item,
//
//     pub struct Decompressor<R: Read>                         (reference src/lib.rs:377-394)
//     pub fn new(r: R) -> Decompressor<R>                      (reference src/lib.rs:398-410)
//     impl<R: Read> Read for Decompressor<R> { fn read(..) }   (reference src/lib.rs:2173-2193)
//
// on top of the C ABI (include/brx.h).  The reference is Rust; this image has no Rust toolchain, so the
// host side that sits above the C ABI is written in C++ with the same shape (INTEGRATION.md shows the Rust
// shim a maintainer of the reference would add).  Header-only; link with -lbrx.
//
//   brotli::Decompressor<brotli::SliceReader> d(brotli::SliceReader(ptr, n));
//   std::vector<uint8_t> out = d.read_to_end();        // == Read::read_to_end
//
// Semantics of read(): n > 0 bytes, 0 at end of stream forever after; an invalid stream throws
// brotli::InvalidData whose what() is the reference's description string (the reference returns
// io::Error::new(ErrorKind::InvalidData, description), src/lib.rs:2177).  Two documented differences of the
// GPU backend: the inner reader of a SHORT stream (compressed input < 4 MiB) is drained eagerly on the first read, a longer one is
// pulled as it decodes -- in bounded device memory whatever the stream holds: the reader's windows grow when ONE command produces
// more than the room behind the output window or ONE item needs more input than the input window (brx.h, brx_stream_new_reader;
// before round 5 such a stream failed over a reader), and the pull callback runs with the context's lock released, so R may itself
// be a Decompressor on default_context(); for a stream that fails the bytes
// produced before the error are delivered first, then the error (the reference delivers an unspecified prefix too,
// SURVEY.md Q13).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/brx.h"

namespace brotli {

struct InvalidData : std::runtime_error {
    int status;
    InvalidData(int st, const char *what) : std::runtime_error(what), status(st) {}
};

// A minimal "Read": any type with  size_t read(uint8_t *buf, size_t len)  returning 0 at EOF works as R.
class SliceReader {
    const uint8_t *p_;
    size_t n_, at_ = 0;

  public:
    SliceReader(const uint8_t *p, size_t n) : p_(p), n_(n) {}
    size_t read(uint8_t *buf, size_t len) {
        size_t k = n_ - at_ < len ? n_ - at_ : len;
        for (size_t i = 0; i < k; i++) buf[i] = p_[at_ + i];
        at_ += k;
        return k;
    }
};

inline brx_ctx *default_context() {
    static brx_ctx *ctx = [] {
        brx_ctx *c = nullptr;
        int rc = brx_ctx_create(&c, 0);
        if (rc != BRX_SUCCESS) throw std::runtime_error(std::string("brx_ctx_create: ") + brx_last_error());
        return c;
    }();
    return ctx;
}

// Decompressor<R>: small streams are drained and POOLED (the first read of any queued Decompressor decodes all of them in one
// batch); a stream whose compressed input does not end within the first 4 MiB is decoded the way the reference does it -- the
// inner reader is PULLED while the stream decodes (brx_stream_new_reader: src/bitreader/mod.rs:21-53), compressed input and
// decoded output both in bounded sliding windows on the device, whatever the stream's length.
template <class R> class Decompressor {
    R inner_;
    brx_stream *stream_ = nullptr;
    std::vector<uint8_t> head_; // what was drained before the stream turned out to be a long one: replayed to the puller first
    size_t head_at_ = 0;

    static size_t pull(void *user, uint8_t *buf, size_t cap) { // brx_read_fn
        Decompressor *d = static_cast<Decompressor *>(user);
        try {
            if (d->head_at_ < d->head_.size()) {
                size_t k = d->head_.size() - d->head_at_ < cap ? d->head_.size() - d->head_at_ : cap;
                for (size_t i = 0; i < k; i++) buf[i] = d->head_[d->head_at_ + i];
                d->head_at_ += k;
                if (d->head_at_ == d->head_.size()) std::vector<uint8_t>().swap(d->head_), d->head_at_ = 0;
                return k;
            }
            return d->inner_.read(buf, cap);
        } catch (...) {
            return 0; // no exception crosses the C ABI: the input ends here
        }
    }

  public:
    static constexpr size_t POOLED_LIMIT = 4u << 20;
    explicit Decompressor(R r) : inner_(std::move(r)) {} // infallible and reads nothing, like the reference's new()
    Decompressor(const Decompressor &) = delete;          // the reference derives Debug only, not Clone
    Decompressor &operator=(const Decompressor &) = delete;
    ~Decompressor() { brx_stream_free(stream_); }

    // Drain the inner reader (up to POOLED_LIMIT) and queue the stream on the context without decoding: the first read() of ANY
    // queued Decompressor then decodes all of them in one batch (brx.h, Read facade).  A longer input becomes a pulled stream.
    void prepare() {
        if (stream_) return;
        std::vector<uint8_t> in;
        uint8_t tmp[65536];
        bool ended = false;
        while (in.size() < POOLED_LIMIT) {
            size_t k = inner_.read(tmp, sizeof tmp);
            if (k == 0) { ended = true; break; }
            in.insert(in.end(), tmp, tmp + k);
        }
        if (ended) {
            stream_ = brx_stream_new(default_context(), in.data(), in.size());
        } else {
            head_.swap(in);
            stream_ = brx_stream_new_reader(default_context(), &Decompressor::pull, this);
        }
        if (!stream_) throw std::runtime_error("brx_stream_new failed");
    }

    size_t read(uint8_t *buf, size_t len) {
        prepare();
        int64_t n = brx_stream_read(stream_, buf, len);
        if (n < -900) throw std::runtime_error(std::string("libbrx: ") + brx_last_error());
        if (n < 0) throw InvalidData((int)-n, brx_status_str((int32_t)-n));
        return (size_t)n;
    }

    // Decoded bytes read() hands out without decoding anything (brx_stream_ready): for hosts that move many streams with advance().
    size_t ready() {
        prepare();
        return (size_t)brx_stream_ready(stream_);
    }
    brx_stream *handle() { // (prepared)
        prepare();
        return stream_;
    }

    std::vector<uint8_t> read_to_end() {
        std::vector<uint8_t> out;
        uint8_t tmp[65536];
        for (size_t k; (k = read(tmp, sizeof tmp)) > 0;) out.insert(out.end(), tmp, tmp + k);
        return out;
    }
};

// Many Decompressors on ONE thread (an event loop over sockets): every one that is pulled (its input did not end within the first
// POOLED_LIMIT bytes), unfinished and has nothing left to read moves on by one slice, all of those slices in shared launches
// (brx_stream_advance; reader rounds in brx.h).  The others are left alone: read() serves them as before.  All must be on
// default_context().  Returns how many moved on.
template <class D> size_t advance(D *const *ds, size_t n) {
    std::vector<brx_stream *> h;
    h.reserve(n);
    for (size_t i = 0; i < n; i++) h.push_back(ds[i]->handle());
    const int rc = brx_stream_advance(h.data(), (uint32_t)h.size());
    if (rc < 0) throw std::runtime_error(std::string("brx_stream_advance: ") + brx_last_error());
    return (size_t)rc;
}
template <class D> size_t advance(const std::vector<D *> &ds) { return advance(ds.data(), ds.size()); }

// The device-memory passes over a decoded batch (BRX_MEM_DEVICE; every pointer is device memory, `stream` a hipStream_t or
// nullptr for the context's own): the decoded bytes back to back, and their CRC-32 / CRC-32C (kind = BRX_DIGEST_*; `expect` and
// `mismatch` both or neither) -- a batch that never leaves the device is verified there.  brx.h has the contracts.
inline void compact_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint8_t *dst,
                          const uint64_t *dst_off, uint64_t total, void *stream = nullptr) {
    if (brx_compact_batch(ctx, out, out_off, len, n, dst, dst_off, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_compact_batch: ") + brx_last_error());
}
inline void digest_batch(brx_ctx *ctx, uint32_t kind, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                         uint32_t *digest, const uint32_t *expect = nullptr, uint32_t *mismatch = nullptr, void *stream = nullptr) {
    if (brx_digest_batch(ctx, kind, out, out_off, len, n, digest, expect, mismatch, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_digest_batch: ") + brx_last_error());
}
// Record boundaries of the same batch: count[i] = bytes equal to `delim` in stream i; with `pos_off` (the exclusive prefix sum of the
// counts) and `pos` (room for `total` entries) also their offsets within the stream, ascending.  `span` = size of the arena behind `out`.
inline void index_batch(brx_ctx *ctx, uint8_t delim, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                        uint64_t span, uint64_t *count, const uint64_t *pos_off = nullptr, uint64_t *pos = nullptr, uint64_t total = 0,
                        void *stream = nullptr) {
    if (brx_index_batch(ctx, delim, out, out_off, len, n, span, count, pos_off, pos, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_index_batch: ") + brx_last_error());
}
// The same with RFC 4180 quoting: a `delim` byte is a record delimiter only where the number of `quote` bytes in front of it in its
// stream is even; open[i] (may be nullptr) = 1 where stream i ends inside a quoted field.  No escape characters, no CR handling.
inline void index_quoted_batch(brx_ctx *ctx, uint8_t delim, uint8_t quote, const uint8_t *out, const uint64_t *out_off, const uint64_t *len,
                               uint32_t n, uint64_t span, uint64_t *count, uint32_t *open = nullptr, const uint64_t *pos_off = nullptr,
                               uint64_t *pos = nullptr, uint64_t total = 0, void *stream = nullptr) {
    if (brx_index_quoted_batch(ctx, delim, quote, out, out_off, len, n, span, count, open, pos_off, pos, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_index_quoted_batch: ") + brx_last_error());
}
// The same for dialects with an escape byte (JSON Lines, SQL text dumps, CSV with an escape character): a byte behind an odd run of
// `escape` bytes is data; a `delim` byte is a record delimiter where it is not escaped and the number of unescaped `quote` bytes in
// front of it is even.  flags = BRX_INDEX_NO_QUOTE: no byte is a quote.  open[i] (may be nullptr): bit 0 = stream i ends inside a
// quoted field, bit 1 = it ends on an escape that has nothing to escape.
inline void index_escaped_batch(brx_ctx *ctx, uint8_t delim, uint8_t quote, uint8_t escape, uint32_t flags, const uint8_t *out,
                                const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint64_t *count,
                                uint32_t *open = nullptr, const uint64_t *pos_off = nullptr, uint64_t *pos = nullptr, uint64_t total = 0,
                                void *stream = nullptr) {
    if (brx_index_escaped_batch(ctx, delim, quote, escape, flags, out, out_off, len, n, span, count, open, pos_off, pos, total, stream) !=
        BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_index_escaped_batch: ") + brx_last_error());
}
// The same with a SET of delimiter bytes (`delims`, HOST memory, 1 .. 8 distinct bytes, e.g. ",\n" or "{}[]:,\n") and with the escape
// as optional as the quote (flags: BRX_INDEX_NO_QUOTE, BRX_INDEX_NO_ESCAPE): a byte of the set is a boundary where it is not escaped
// and outside quotes; what[pos_off[i] + k] (may be nullptr, only with `pos`) = the byte that stands at pos[pos_off[i] + k].
inline void index_set_batch(brx_ctx *ctx, const uint8_t *delims, uint32_t n_delims, uint8_t quote, uint8_t escape, uint32_t flags,
                            const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint64_t *count,
                            uint32_t *open = nullptr, const uint64_t *pos_off = nullptr, uint64_t *pos = nullptr, uint8_t *what = nullptr,
                            uint64_t total = 0, void *stream = nullptr) {
    if (brx_index_set_batch(ctx, delims, n_delims, quote, escape, flags, out, out_off, len, n, span, count, open, pos_off, pos, what,
                            total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_index_set_batch: ") + brx_last_error());
}
// Occurrences of a byte sequence (`needle`, HOST memory, 1 .. 16 bytes, e.g. "\r\n") in the same batch: count[i] = occurrences in
// stream i, overlapping ones included; with `pos_off` and `pos` also the offset within the stream of each one's first byte, ascending.
inline void find_batch(brx_ctx *ctx, const uint8_t *needle, uint32_t needle_len, const uint8_t *out, const uint64_t *out_off,
                       const uint64_t *len, uint32_t n, uint64_t span, uint64_t *count, const uint64_t *pos_off = nullptr,
                       uint64_t *pos = nullptr, uint64_t total = 0, void *stream = nullptr) {
    if (brx_find_batch(ctx, needle, needle_len, out, out_off, len, n, span, count, pos_off, pos, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_find_batch: ") + brx_last_error());
}
// The selected records of the same batch, from the positions of any of the passes above (`delim_len` = 1, or the needle's length):
// entry j is record sel_rec[j] of stream sel_stream[j], or with both nullptr every record of every stream in turn.  Size mode
// (dst_off, dst nullptr): rec_len[j] = the record's length.  Fill mode: its bytes at dst[dst_off[j] ..], cut at the entry's room.
// flags: BRX_TAKE_NO_DELIM, BRX_TAKE_TRIM_CR.
inline void take_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                       const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                       uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint64_t *rec_len,
                       const uint64_t *dst_off = nullptr, uint8_t *dst = nullptr, uint64_t total = 0, void *stream = nullptr) {
    if (brx_take_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, rec_len,
                       dst_off, dst, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_take_batch: ") + brx_last_error());
}
// A 64-bit key of every selected record (the selection, the positions and the flags as for take_batch): hash[j] under `seed`, equal
// for equal records, 0 for the empty one; rec_len (optional) as take_batch's size mode writes it.
inline void hash_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                       const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                       uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint64_t seed, uint64_t *hash,
                       uint64_t *rec_len = nullptr, void *stream = nullptr) {
    if (brx_hash_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, seed, hash,
                       rec_len, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_hash_batch: ") + brx_last_error());
}
// Every selected record as a 64-bit number (the selection, the positions and the BRX_TAKE_* flags as for take_batch; BRX_PARSE_SPACES /
// BRX_PARSE_QUOTED in the same flags word): val[j] and status[j] (BRX_PARSE_OK .. BRX_PARSE_LONG) for `kind` BRX_PARSE_INT, BRX_PARSE_DEC
// (x * 10^scale truncated toward zero, scale 0 .. 18) or BRX_PARSE_HEX.  Exact integer arithmetic; records above 64 bytes are LONG.
inline void parse_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                        const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                        uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint32_t kind, uint32_t scale,
                        uint8_t quote, int64_t *val, uint8_t *status, void *stream = nullptr) {
    if (brx_parse_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, kind, scale,
                        quote, val, status, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_parse_batch: ") + brx_last_error());
}
// Every selected record as a correctly rounded double (the selection, the positions and the BRX_TAKE_* flags as for take_batch;
// BRX_PARSE_SPACES / BRX_PARSE_QUOTED / BRX_PARSE_WORDS in the same flags word): val[j] and status[j] (BRX_PARSE_OK, _EMPTY, _RANGE, _BAD,
// _LONG, or _HARD: val[j] or the next double away from zero, to be finished by the caller).  Exponents; records above 64 bytes are LONG.
inline void parse_f64_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                            const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                            uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint8_t quote, double *val,
                            uint8_t *status, void *stream = nullptr) {
    if (brx_parse_f64_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, quote, val,
                            status, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_parse_f64_batch: ") + brx_last_error());
}
// Every selected record as a date, a time of day or a timestamp (the selection, the positions and the BRX_TAKE_* flags as for take_batch;
// BRX_PARSE_SPACES / BRX_PARSE_QUOTED in the same flags word): kind BRX_TIME_DATE (val[j] = days since 1970-01-01), BRX_TIME_TIME or
// BRX_TIME_STAMP (val[j] = units of 10^-scale s, scale 0 .. 9, rounded toward minus infinity), status[j] (BRX_PARSE_OK, _INEXACT, _EMPTY,
// _RANGE, _BAD, _LONG) and, if zone is given, zone[j] = the offset in minutes east of UTC or BRX_TIME_NO_ZONE.  ISO 8601 / RFC 3339 in
// the extended format only; records above 64 bytes are LONG.
inline void parse_time_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                             const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                             uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint32_t kind, uint32_t scale,
                             uint8_t quote, int64_t *val, uint8_t *status, int16_t *zone = nullptr, void *stream = nullptr) {
    if (brx_parse_time_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, kind, scale,
                             quote, val, status, zone, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_parse_time_batch: ") + brx_last_error());
}
// Every selected record as the string it spells (the selection, the positions and the BRX_TAKE_* flags as for take_batch; BRX_PARSE_SPACES
// in the same flags word): dialect BRX_TEXT_CSV (an enclosing pair of `quote`, two of them inside it are one), BRX_TEXT_JSON (string
// escapes, \uXXXX and surrogate pairs as UTF-8) or BRX_TEXT_BACKSLASH (COPY text; `escape` 'N' alone is BRX_TEXT_NULL).  Size mode
// (dst_off, dst nullptr): text_len[j] and status[j] (BRX_TEXT_OK, _BARE, _NULL, _BAD).  Fill mode: the text at dst[dst_off[j] ..], cut
// at the entry's room; text_len and status may then be nullptr.  A text is never longer than its record.
inline void unescape_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                           const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos, uint32_t delim_len,
                           uint32_t flags, const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint32_t dialect, uint32_t quote,
                           uint32_t escape, uint64_t *text_len, uint8_t *status, const uint64_t *dst_off = nullptr, uint8_t *dst = nullptr,
                           uint64_t total = 0, void *stream = nullptr) {
    if (brx_unescape_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m, dialect, quote,
                           escape, text_len, status, dst_off, dst, total, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_unescape_batch: ") + brx_last_error());
}
// The named members of the JSON Lines objects of a batch as selections for the calls above: count, pos_off, pos, what and n_pos as a
// fill-mode brx_index_set_batch call with the delimiters { } [ ] : , and the line feed left them; names (host memory) holds name q at
// names[32 q .. 32 q + name_len[q]).  Count mode (line_off, sel_stream, sel_rec, kind nullptr): lines[i].  Fill mode: entry (q, j) at
// q * m + j is the last depth-1 member of line j whose key is name q: sel_stream / sel_rec as the record calls take them, kind
// BRX_MEMBER_MISSING ... BRX_MEMBER_BAD; line_flags[j] (may be nullptr) BRX_MEMBER_LONG_KEY | _ESCAPED_KEY | _UNBALANCED.
inline void member_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                         const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                         const uint8_t *names, const uint32_t *name_len, uint32_t n_names, uint64_t *lines, const uint64_t *line_off = nullptr,
                         uint64_t m = 0, uint32_t *sel_stream = nullptr, uint64_t *sel_rec = nullptr, uint8_t *kind = nullptr,
                         uint8_t *line_flags = nullptr, void *stream = nullptr) {
    if (brx_member_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, what, n_pos, names, name_len, n_names, lines, line_off, m,
                         sel_stream, sel_rec, kind, line_flags, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_member_batch: ") + brx_last_error());
}
// The elements of the JSON arrays whose openers (sel_stream, sel_rec) name -- a column of member_batch's output, sel_rec the boundary of
// the '[' -- as a selection for the record calls.  Count mode (el_off, el_stream, el_rec, el_kind nullptr): n_elem[j], status[j]
// (BRX_ELEMENTS_OK ... BRX_ELEMENTS_MISMATCH, may be nullptr) and end[j] (the closer's boundary, may be nullptr).  Fill mode: element t
// of entry j at el_off[j] + t, inside the entry's room and below total: el_stream / el_rec as the record calls take them, el_kind
// BRX_MEMBER_SCALAR ... BRX_MEMBER_BAD; n_elem may be nullptr.
inline void elements_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                           const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                           const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, uint64_t *n_elem, uint8_t *status = nullptr,
                           uint64_t *end = nullptr, const uint64_t *el_off = nullptr, uint64_t total = 0, uint32_t *el_stream = nullptr,
                           uint64_t *el_rec = nullptr, uint8_t *el_kind = nullptr, void *stream = nullptr) {
    if (brx_elements_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, what, n_pos, sel_stream, sel_rec, m, n_elem, status, end,
                           el_off, total, el_stream, el_rec, el_kind, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_elements_batch: ") + brx_last_error());
}
// The named members of the nested JSON objects whose openers (sel_stream, sel_rec) name -- a column of member_batch's output or
// elements_batch's el_stream / el_rec, sel_rec the boundary of the '{'; entries that are no such opener may stay in it.  names (host
// memory) as for member_batch.  Entry (q, j) at q * m + j is the last member of object j whose key is name q: mem_stream / mem_rec as
// the record calls take them, mem_kind BRX_MEMBER_MISSING ... BRX_MEMBER_BAD (OBJECT: again an opener for this call; ARRAY: one for
// elements_batch); n_members[j], status[j] (BRX_OBJECT_OK ... BRX_OBJECT_MISMATCH), end[j] (the closer's boundary) and obj_flags[j]
// (BRX_MEMBER_LONG_KEY | _ESCAPED_KEY) may each be nullptr.  n_names = 0 is the extent mode: n_members, status and end alone.
inline void object_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                         const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                         const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m, const uint8_t *names, const uint32_t *name_len,
                         uint32_t n_names, uint64_t *n_members, uint8_t *status = nullptr, uint64_t *end = nullptr,
                         uint32_t *mem_stream = nullptr, uint64_t *mem_rec = nullptr, uint8_t *mem_kind = nullptr,
                         uint8_t *obj_flags = nullptr, void *stream = nullptr) {
    if (brx_object_batch(ctx, out, out_off, len, n, span, count, pos_off, pos, what, n_pos, sel_stream, sel_rec, m, names, name_len, n_names,
                         n_members, status, end, mem_stream, mem_rec, mem_kind, obj_flags, stream) != BRX_SUCCESS)
        throw std::runtime_error(std::string("brx_object_batch: ") + brx_last_error());
}

} // namespace brotli
