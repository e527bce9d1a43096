// brx_unescape.hip -- brx_unescape_batch: every selected record of the decoded streams of a batch as the string it spells (CSV quoting,
// JSON string escapes, backslash escapes), as lengths and statuses (size mode) or as bytes in a destination (fill mode).  The plan of a
// record, the classification of a unit, the escapes, the walk of a unit and the lane path are plain C++ in brx_unescape.h, shared with
// tools/unescape_emu.cpp; the record rule is that of brx_take.h.  This file holds what is HIP and its own: the ballot over the long
// records, the carries and the sums across the wave, and the launch.  What the record kernels share on the device is brx_record_dev.h
// (DESIGN.md 17.1).
//
// One lane owns one entry.  A record whose walk range is shorter than BRX_TEXT_LONG is walked by its lane alone, unit by unit.  The
// lanes with longer ones leave them out; the wave then takes those one at a time in a wave-uniform loop over their ballot, lane l on
// unit 64 row + l: the run parity goes from lane to lane by a ballot and a shuffle, a lane's place in the text by a prefix sum of the
// lanes' output counts.  The kernel is compiled once per dialect, so that the unit walk holds one dialect's tokens only.  No scratch,
// no atomics, no LDS.
#include "brx_record_dev.h"
#include "brx_unescape.h"

// x of lane `src` as every lane's own copy, in a vector register.  What the unit walk reads of the record in hand (its address, its
// range, its room) is taken this way and not by readlane: as scalars, together with the saved execution masks of the walk's branches,
// they do not fit the scalar registers of a wave, and the compiler spills them.  Only the row loop's own bounds are scalars
// (brx_rec_bcast).
__device__ __forceinline__ uint64_t brx_text_copy(uint64_t x, uint32_t src) { return (uint64_t)__shfl((unsigned long long)x, (int)src, 64); }

template <uint32_t DIALECT>
__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_unescape_kernel(BrxTakeArgs a, BrxTextArgs x) {
    // every lane stays to the end: the loop over the long records needs the whole wave
    const uint64_t j = brx_rec_entry();
    const uint32_t lane = threadIdx.x & 63u;
    constexpr uint32_t MODE = DIALECT + 1u; // BRX_TEXT_M_* of a record that is not copied as it stands
    BrxRecMemUnaligned mem; // (a text's bytes go out wherever they fall)
    BrxTakeRec r = {0, 0};
    BrxTextPlan p = {0, 0, BRX_TEXT_M_COPY, BRX_TEXT_S_BARE};
    BrxTextRoom d = {0, 0};
    BrxTextRes res = {0, 0, 0};
    const bool serial = brx_text_hex_escape(DIALECT, x.e); // (wave-uniform)
    bool is_long = false;
    if (j < a.m) {
        r = brx_take_entry_record(mem, a, j);
        p = brx_text_plan(mem, a.out + r.src, (int64_t)r.len, a.flags, DIALECT, x.q, x.e);
        d = brx_text_room(x, a.m, j);
        if (serial && p.mode == BRX_TEXT_M_JSON) res = brx_text_serial(mem, a.out + r.src, (int64_t)r.len, p, x.q, x.e, d);
        else if (p.we - p.ws >= (int64_t)BRX_TEXT_LONG) is_long = true;
        else res = brx_text_lane<MODE>(mem, a.out + r.src, (int64_t)r.len, p, x.q, x.e, d);
    }
    uint64_t todo = __ballot(is_long);
    while (todo) { // (wave-uniform)
        const uint32_t owner = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1u;
        const uint8_t *rec = a.out + brx_text_copy(r.src, owner);
        const int64_t L = (int64_t)brx_text_copy(r.len, owner);
        BrxTextPlan wp;
        wp.ws = (int64_t)brx_text_copy((uint64_t)p.ws, owner);
        wp.we = (int64_t)brx_text_copy((uint64_t)p.we, owner);
        const int64_t u_ws = (int64_t)brx_rec_bcast((uint64_t)p.ws, owner), u_we = (int64_t)brx_rec_bcast((uint64_t)p.we, owner);
        wp.mode = brx_rec_bcast32(p.mode, owner);
        wp.status = 0;
        uint8_t *dstp = (uint8_t *)brx_text_copy((uint64_t)(uintptr_t)d.dstp, owner);
        const uint64_t room = brx_text_copy(d.room, owner);
        uint64_t base = 0;
        uint32_t bad = 0, closed = 0;
        BrxTextCarry carry = {0, 0};
        for (int64_t row = brx_text_row0(u_ws); row < u_we; row += BRX_TEXT_ROW) {
            const int64_t b = row + (int64_t)lane * BRX_TEXT_UNIT;
            const BrxTextPre u = brx_text_pre<MODE>(mem, rec, L, wp, x.q, x.e, b);
            const uint32_t e0 = brx_text_ebits(u.em, 0u);
            const int32_t src = brx_text_pin_lane(__ballot(u.em != 0xFFFFu), lane);
            const uint32_t E = brx_text_row_e(u.em, e0, src, (uint32_t)__shfl((int)e0, src < 0 ? 0 : src, 64), carry);
            const uint32_t Eprev = brx_text_row_prev(lane, (uint32_t)__shfl_up((int)E, 1, 64), carry);
            carry = brx_text_row_carry(brx_rec_bcast32(E, 63u));
            const BrxTextOut o = brx_text_unit<MODE>(mem, rec, L, wp, x.q, x.e, b, u, Eprev | (E << 16));
            uint32_t sum = o.cnt; // inclusive prefix sum of the lanes' counts
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)sum, s, 64);
                if (lane >= (uint32_t)s) sum += y;
            }
            brx_text_store(mem, dstp, brx_text_row_at(base, sum, o.cnt), room, o);
            base += brx_rec_bcast32(sum, 63u);
            bad |= __ballot(o.bad != 0u) != 0u;
            closed |= __ballot(o.closed != 0u) != 0u;
        }
        if (lane == owner) { res.len = base; res.bad = bad; res.closed = closed; }
    }
    if (j < a.m) {
        if (x.text_len) x.text_len[j] = res.len;
        if (x.status) x.status[j] = (uint8_t)brx_text_status(p, res.bad, res.closed);
    }
}

void brx_launch_unescape(const BrxTakeArgs &a, const BrxTextArgs &x, void *hip_stream) {
    if (a.m == 0) return;
    const dim3 grid(brx_rec_blocks(a.m)), block(BRX_REC_BLOCK);
    if (x.dialect == BRX_TEXT_D_CSV) hipLaunchKernelGGL(brx_unescape_kernel<BRX_TEXT_D_CSV>, grid, block, 0, (hipStream_t)hip_stream, a, x);
    else if (x.dialect == BRX_TEXT_D_JSON) hipLaunchKernelGGL(brx_unescape_kernel<BRX_TEXT_D_JSON>, grid, block, 0, (hipStream_t)hip_stream, a, x);
    else hipLaunchKernelGGL(brx_unescape_kernel<BRX_TEXT_D_BACKSLASH>, grid, block, 0, (hipStream_t)hip_stream, a, x);
}
