// dpt_host_layout.h -- where each host-buffer call (dpt_host.cpp) keeps its arrays in the ctx's two staging
// buffers, "in" (copied to the device) and "out" (copied back).  Pure arithmetic, no HIP: testable without a
// device (dpt_debug_host_layout, tests/test_host_layout.py).
#pragma once
#include <stdint.h>

namespace dpt {

// One array of a side: `payload` bytes the call copies, then `slack` bytes the kernels may still read -- the
// NUL after a text or cut mask, one dword after ids and statuses (they load whole dwords) -- at an 8-byte
// aligned offset.  An absent optional array has neither and takes no room.
struct Segment {
    uint64_t offset, payload, slack;
};
constexpr int HOST_MAX_SEG = 7;
struct HostSide {
    Segment seg[HOST_MAX_SEG];
    int n = 0;
    uint64_t bytes = 0;   // the end of the last segment, rounded up to 8
    HostSide &add(uint64_t payload, uint64_t slack, bool present = true) {
        seg[n++] = {bytes, present ? payload : 0, present ? slack : 0};
        if (present) bytes += (payload + slack + 7) & ~7ull;
        return *this;
    }
    HostSide &bytes8(uint64_t n_el, bool present = true) { return add(n_el, 1, present); }        // text, cut mask, decoded bytes
    HostSide &int32s(uint64_t n_el, bool present = true) { return add(4 * n_el, 4, present); }    // ids, statuses, spans
    HostSide &offsets(uint64_t n_str) { return add(8 * (n_str + 1), 0); }                         // a CSR offset array
};
struct HostLayout {
    HostSide in, out;
};

// The segments of each call in their order, the in side's, then (from 0 again) the out side's.
enum EncodeSeg { ENC_TEXT, ENC_STR_OFF, ENC_CUT, ENC_ID_OFF = 0, ENC_STATUS, ENC_CAPPED, ENC_CTR, ENC_IDS, ENC_EDGES, ENC_FAR };
enum SpansSeg { SP_STR_OFF, SP_ID_OFF, SP_IDS, SP_STATUS, SP_TEXT, SP_CUT, SP_TOK_END = 0, SP_TOK_WORD, SP_SPAN_STATUS };
enum DecodeSeg { DEC_ID_OFF, DEC_OUT_OFF, DEC_IDS, DEC_STATUS, DEC_RESULT = 0, DEC_BYTES, DEC_OUT_LEN };
enum RoundtripSeg { RT_ID_OFF, RT_STR_OFF, RT_IDS, RT_STATUS, RT_TEXT, RT_RESULT = 0, RT_FIRST_DIFF };

// The text sits at 0 of the in side (a zero-copy call passes the buffer itself as the text).  The head of the
// out side -- id_off | status | capped | the counter block's 64-byte snapshot -- sits ahead of the ids: a large
// call copies the head back first and then only the ids it produced, a small one everything at once.
inline HostLayout encode_layout(uint64_t n_bytes, uint64_t n_str, bool cut, bool edges, uint64_t far_pairs) {
    HostLayout l;
    l.in.bytes8(n_bytes).offsets(n_str).bytes8(n_bytes, cut);
    l.out.offsets(n_str).int32s(n_str).int32s(n_str).add(64, 0).int32s(n_bytes).add(8 * n_bytes, 8, edges).add(16 * far_pairs, 0);
    return l;
}
inline HostLayout spans_layout(uint64_t n_bytes, uint64_t n_str, uint64_t n_tok, bool cut, bool tok_word) {
    HostLayout l;
    l.in.offsets(n_str).offsets(n_str).int32s(n_tok).int32s(n_str).bytes8(n_bytes).bytes8(n_bytes, cut);
    l.out.int32s(n_tok).int32s(n_tok, tok_word).int32s(n_str);
    return l;
}
// dpt_decode_host stages twice: for the sizes pass with decoded = 0 (it reads out_len back), then with the
// decoded bytes' count for the decode pass (dec_status and the bytes: the prefix of the out side).  The in
// side is the same both times.
inline HostLayout decode_layout(uint64_t n_str, uint64_t n_tok, uint64_t decoded) {
    HostLayout l;
    l.in.offsets(n_str).offsets(n_str).int32s(n_tok).int32s(n_str);
    l.out.int32s(n_str).bytes8(decoded).add(8 * n_str, 0);
    return l;
}
inline HostLayout roundtrip_layout(uint64_t n_bytes, uint64_t n_str, uint64_t n_tok) {
    HostLayout l;
    l.in.offsets(n_str).offsets(n_str).int32s(n_tok).int32s(n_str).bytes8(n_bytes);
    l.out.int32s(n_str).int32s(n_str);
    return l;
}

}  // namespace dpt
