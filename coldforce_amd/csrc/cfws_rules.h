// cfws_rules.h -- reference rules that both the device units and the host
// units (cfws_pipeline.cpp, cfws_frame.cpp) apply, each written once so the
// two sides cannot drift apart.
#ifndef CFWS_RULES_H
#define CFWS_RULES_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "cfws.h"

// WS header bytes of a frame with an n-byte payload (co_ws_frame.c:41-91).
__host__ __device__ __forceinline__ uint32_t header_size_of(uint64_t n, bool mask)
{
    return 2u + (n > 65535u ? 8u : (n > 125u ? 2u : 0u)) + (mask ? 4u : 0u);
}

// DATA frames that W wire bytes become: co_http2_stream_send_data splits them
// into frames of at most max_frame_size S, and sends one empty frame for no
// bytes (co_http2_stream.c:964-1010).
__host__ __device__ __forceinline__ uint64_t data_frames_of(uint64_t W, uint64_t S)
{
    return W <= S ? 1 : (W + S - 1) / S;
}

// The HTTP/2 frame at offset s of h2[0, size) (co_http2_frame.c:211-300):
// MORE_DATA under 9 bytes, PARSE_ERROR when length > max_frame_size,
// MORE_DATA when the payload is incomplete, CFWS_H2_NOT_DATA for other types
// (no bytes), PARSE_ERROR for bad padding. The byte reads keep the
// reference's order: it decides which status wins. type and end_stream (the
// flags' END_STREAM bit, the only flag read after the decision: carrying the
// whole byte cost the receive's reduce kernel a register) hold what was read
// before the decision; header_size (9, or 10 with a pad length
// byte) and payload_size (the DATA payload without pad length and padding)
// are set for a COMPLETE frame only.
struct H2Frame {
    int32_t status;
    uint8_t type, end_stream, header_size;
    uint64_t payload_size;
};

__host__ __device__ __forceinline__ H2Frame h2_frame_at(const uint8_t* __restrict__ h2, uint64_t size,
                                                        uint64_t s, uint64_t max_frame)
{
    H2Frame r = {};
    int32_t st = CFWS_H2_PARSE_COMPLETE;
    do {
        if (s > size || size - s < 9) { st = CFWS_H2_PARSE_MORE_DATA; break; }
        const uint64_t len = (uint64_t)h2[s] << 16 | (uint64_t)h2[s + 1] << 8 | h2[s + 2];
        if (len > max_frame) { st = CFWS_H2_PARSE_ERROR; break; }
        if (size - s - 9 < len) { st = CFWS_H2_PARSE_MORE_DATA; break; }
        r.type = h2[s + 3];
        const uint32_t flags = h2[s + 4];
        r.end_stream = (uint8_t)(flags & 0x1u);
        if (r.type != 0) { st = CFWS_H2_NOT_DATA; break; }
        uint64_t pad = 0, hs = 9;
        if (flags & 0x8u) {                             // PADDED
            if (len < 1) { st = CFWS_H2_PARSE_ERROR; break; }
            pad = h2[s + 9];
            hs = 10;
            if (pad + 1 > len) { st = CFWS_H2_PARSE_ERROR; break; }
        }
        r.header_size = (uint8_t)hs;
        r.payload_size = len - (hs - 9) - pad;
    } while (0);
    r.status = st;
    return r;
}

// One hop of the HTTP/2 receive loop (co_http2_client_on_tcp_receive_ready,
// co_http2_client.c:462-541, around co_http2_frame_deserialize,
// co_http2_frame.c:211-533): the frame whose first bytes are b[0..9] (the
// 9-byte header, then the pad length when there is one), with `avail` bytes
// left in the buffer (> 0: the loop ends at 0 before any parse), under
// max_frame. at(i) is byte i; it is asked for byte i only when i < avail and,
// for byte 9, only when PADDED is set and length >= 1. The decisions keep the
// reference's order, which decides what wins:
//   avail < 9 -> MORE_DATA; length > max_frame -> ERROR (:244-247, before the
//   completeness check); avail - 9 < length -> MORE_DATA (:249-253);
//   type > 9 -> ERROR (:524-527).
// Then `need`, the payload bytes the type's fixed fields take (pad length +
// padding, priority, promised stream id, the fixed-size payloads). Where
// need > length the reference subtracts past zero in an unsigned length
// (:281, :316, :331, :445, :483) or reads past the frame into whatever
// follows and trips its caller's co_assert (co_http2_client.c:471): its
// behaviour is undefined there. ERROR is THIS LIBRARY'S rule for those frames
// (as h2_frame_at already decides for DATA), not the reference's.
// advance is what the parse consumed (`(*index) += data_ptr - data_head`,
// :530), which is not 9 + length for the fixed-size types: they step over
// their fields only, and SETTINGS over 6 bytes per parameter of a count cast
// to uint16_t (:391-392). stream_id keeps the reserved bit (:263-265).
// Fields other than status are set for a COMPLETE frame only.
struct H2Hop {
    int32_t status;
    uint32_t stream_id, length, advance;
    uint8_t type, flags;
};

template <typename At>
__host__ __device__ __forceinline__ H2Hop h2_hop_by(At at, uint64_t avail, uint32_t max_frame)
{
    H2Hop r = {};
    r.status = CFWS_H2_PARSE_MORE_DATA;
    if (avail < 9) return r;
    const uint32_t len = at(0) << 16 | at(1) << 8 | at(2);
    if (len > max_frame) { r.status = CFWS_H2_PARSE_ERROR; return r; }
    if (avail - 9 < len) return r;
    const uint32_t type = at(3), flags = at(4);
    r.status = CFWS_H2_PARSE_ERROR;
    if (type > 9) return r;
    // types with a pad length under PADDED: DATA, HEADERS, PUSH_PROMISE
    uint32_t need = 0;
    if ((type == 0 || type == 1 || type == 5) && (flags & 0x8u)) {
        if (len < 1) return r;
        need = 1u + at(9);
    }
    uint32_t adv = 9u + len;
    switch (type) {
    case 1: need += (flags & 0x20u) ? 5u : 0u; break;            // HEADERS + PRIORITY
    case 2: need = 5; adv = 14; break;                           // PRIORITY
    case 3: need = 4; adv = 13; break;                           // RST_STREAM
    case 4: adv = 9u + 6u * ((len / 6u) & 0xffffu); break;       // SETTINGS
    case 5: need += 4; break;                                    // PUSH_PROMISE
    case 6: need = 8; adv = 17; break;                           // PING
    case 7: need = 8; break;                                     // GOAWAY
    case 8: need = 4; adv = 13; break;                           // WINDOW_UPDATE
    default: break;                                              // DATA, CONTINUATION
    }
    if (need > len) return r;
    r.status = CFWS_H2_PARSE_COMPLETE;
    r.stream_id = at(5) << 24 | at(6) << 16 | at(7) << 8 | at(8);
    r.length = len;
    r.advance = adv;
    r.type = (uint8_t)type;
    r.flags = (uint8_t)flags;
    return r;
}

// Is the COMPLETE frame h reported? (select: CFWS_H2_INDEX_ALL / _DATA;
// stream_id 0: every stream, else the id as read, reserved bit included)
__host__ __device__ __forceinline__ bool h2_selected(const H2Hop& h, uint32_t select, uint32_t stream_id)
{
    return (select == CFWS_H2_INDEX_ALL || h.type == 0) && (stream_id == 0 || h.stream_id == stream_id);
}

// The message rule of cfws_messages_from_frames / cfws_messages_batch
// (include/cfws.h): which received frames make up which message. THIS
// LIBRARY'S rule, not the reference's: the reference hands every frame to the
// application as it arrives (examples/ws_client/main.c:50-72; opcodes
// co_ws_frame.h:28-34) and checks no fragment order. A connection's frames
// are taken in index order with one bit of state, `open` (a message is
// unfinished; false at the connection's start):
//   * message_frame_class: a frame whose header did not parse to a frame is
//     IGNORED (changes nothing, listed nowhere); opcode >= 8 is CONTROL (its
//     index goes to the control list, `open` untouched: control frames may
//     sit between a message's fragments, RFC 6455 5.4); the rest is DATA, the
//     split CFWS_DESERIALIZE_REASSEMBLE uses;
//   * message_starts: a data frame starts a message when it carries an opcode
//     or no message is open, else it joins the open one; then open = !fin;
//   * message_start_flags: a message started by a CONTINUATION is HEADLESS;
//   * message_end_flags: a message ends FINAL with a fin fragment, CUT when
//     another message of its connection starts while it is open, OPEN when
//     its connection's frames end first; LOST_BYTES when a fragment's status
//     is OUT_OF_MEMORY.
// The host form walks with these; the device form (cfws_messages.hip) turns
// `open` into "the connection's previous data frame's fin" and the rest into
// sums, and takes every decision from the same four functions.
enum : uint32_t { kMessageFrameIgnored = 0, kMessageFrameControl = 1, kMessageFrameData = 2 };

__host__ __device__ __forceinline__ uint32_t message_frame_class(int32_t status, uint32_t opcode)
{
    if (status != CFWS_PARSE_COMPLETE && status != CFWS_ERROR_OUT_OF_MEMORY) return kMessageFrameIgnored;
    return opcode >= 8u ? kMessageFrameControl : kMessageFrameData;
}

__host__ __device__ __forceinline__ bool message_starts(uint32_t opcode, bool open)
{
    return opcode != 0u || !open;
}

__host__ __device__ __forceinline__ uint32_t message_start_flags(uint32_t opcode)
{
    return opcode == 0u ? CFWS_MESSAGE_HEADLESS : 0u;
}

// last_fin: the message's last fragment's fin; followed: another message of
// the same connection starts after it; lost: a fragment was OUT_OF_MEMORY
__host__ __device__ __forceinline__ uint32_t message_end_flags(bool last_fin, bool followed, bool lost)
{
    return (last_fin ? CFWS_MESSAGE_FINAL : (followed ? CFWS_MESSAGE_CUT : CFWS_MESSAGE_OPEN)) |
           (lost ? CFWS_MESSAGE_LOST_BYTES : 0u);
}

// The stream rule of cfws_h2_streams_from_frames / cfws_h2_streams_batch
// (include/cfws.h): which indexed HTTP/2 records pool into which message. The
// reference looks a DATA frame's stream up by the id as read
// (co_http2_client.c:475-476), sends stream 0 to the system handler
// (:492-495) and pools every other DATA frame in its stream until END_STREAM
// delivers (co_http2_stream.c:550-608):
//   * h2_stream_pooled: only DATA (type 0) on a stream other than 0 is pooled;
//     every other record is ignored;
//   * a connection's pooled records are taken grouped by stream id (unsigned,
//     as read), arrival order inside a stream; in that order
//     h2_stream_starts: a frame starts a message (or the stream's tail) when
//     it is its connection's first, when the stream changes or when the
//     frame before it carried END_STREAM (h2_stream_closes);
//   * a run that ends with END_STREAM is a closed message, any other run is
//     its stream's tail; h2_stream_msg_flags: a closed message that is the
//     first run of its (connection, stream) is FIRST, a run with a PADDED
//     frame (flag 0x8) is PADDED.
// The host form sorts and walks with these; the device form
// (cfws_h2streams.hip) sorts, then takes the same decisions per row.
constexpr uint32_t kH2FlagEndStream = 0x1u, kH2FlagPadded = 0x8u;

__host__ __device__ __forceinline__ bool h2_stream_pooled(uint32_t type, uint32_t stream_id)
{
    return type == 0u && stream_id != 0u;
}

__host__ __device__ __forceinline__ bool h2_stream_closes(uint32_t flags)
{
    return (flags & kH2FlagEndStream) != 0u;
}

__host__ __device__ __forceinline__ bool h2_stream_starts(bool first_of_conn, bool same_stream, bool prev_closes)
{
    return first_of_conn || !same_stream || prev_closes;
}

// closed: the run's last frame closes; stream_start: the run is the first of
// its (connection, stream); padded: some frame of it has PADDED
__host__ __device__ __forceinline__ uint32_t h2_stream_msg_flags(bool closed, bool stream_start, bool padded)
{
    return (closed ? CFWS_H2_STREAM_CLOSED | (stream_start ? CFWS_H2_STREAM_FIRST : 0u) : CFWS_H2_STREAM_TAIL) |
           (padded ? CFWS_H2_STREAM_PADDED : 0u);
}

// The UTF-8 rule of cfws_utf8_check_messages / cfws_utf8_messages_batch
// (include/cfws.h). THIS LIBRARY'S rule, not the reference's, which validates
// no text; the standard defines it (Unicode Table 3-7, RFC 3629). It is
// written position by position, so that a kernel lane decides every byte from
// the 3 bytes before and the 3 after it and nothing scans over the bytes:
//   * a byte outside 80..BF is a lead; utf8_lead_need: the continuation bytes
//     it needs, kUtf8BadLead for C0, C1, F5..FF (and for "no byte");
//   * utf8_lead_class: a lead is fine when its next `need` bytes exist and are
//     80..BF, the second one narrowed by utf8_second_ok (no overlong forms,
//     no surrogates, nothing above U+10FFFF); TRUNCATED when the bytes that
//     exist pass but some are missing, else INVALID;
//   * utf8_cont_owned: a continuation byte is fine when, walking back up to 3
//     bytes, the first non-continuation byte is a lead that needs at least
//     that many.
// The longest well-formed prefix of a string ends at the smallest position
// that is not fine, and the string is truncated iff that position is a
// truncated lead. The host form walks with utf8_at_by; the device form
// (cfws_utf8.hip) calls utf8_at on a lane's window of bytes; both make the
// result row with utf8_selected, utf8_carried and utf8_row.
constexpr uint32_t kUtf8Absent = 0x100u;        // no byte at this position
constexpr uint32_t kUtf8BadLead = 4u;
enum : uint32_t { kUtf8Fine = 0, kUtf8Invalid = 1, kUtf8Truncated = 2 };

__host__ __device__ __forceinline__ bool utf8_is_cont(uint32_t b) { return (b & 0x1c0u) == 0x80u; }

__host__ __device__ __forceinline__ uint32_t utf8_lead_need(uint32_t b)
{
    return b < 0x80u ? 0u : (b < 0xc2u ? kUtf8BadLead : (b < 0xe0u ? 1u : (b < 0xf0u ? 2u : (b < 0xf5u ? 3u : kUtf8BadLead))));
}

__host__ __device__ __forceinline__ bool utf8_second_ok(uint32_t lead, uint32_t b)
{
    const uint32_t lo = lead == 0xe0u ? 0xa0u : (lead == 0xf0u ? 0x90u : 0x80u);
    const uint32_t hi = lead == 0xedu ? 0x9fu : (lead == 0xf4u ? 0x8fu : 0xbfu);
    return b >= lo && b <= hi;
}

// The lead b with the bytes n1, n2, n3 after it (kUtf8Absent past the end).
__host__ __device__ __forceinline__ uint32_t utf8_lead_class(uint32_t b, uint32_t n1, uint32_t n2, uint32_t n3)
{
    const uint32_t need = utf8_lead_need(b);
    if (need == 0u) return kUtf8Fine;
    if (need == kUtf8BadLead) return kUtf8Invalid;
    if (n1 == kUtf8Absent) return kUtf8Truncated;
    if (!utf8_second_ok(b, n1)) return kUtf8Invalid;
    if (need == 1u) return kUtf8Fine;
    if (n2 == kUtf8Absent) return kUtf8Truncated;
    if (!utf8_is_cont(n2)) return kUtf8Invalid;
    if (need == 2u) return kUtf8Fine;
    if (n3 == kUtf8Absent) return kUtf8Truncated;
    return utf8_is_cont(n3) ? kUtf8Fine : kUtf8Invalid;
}

// A continuation byte with the bytes p1, p2, p3 before it (p1 the nearest).
__host__ __device__ __forceinline__ bool utf8_cont_owned(uint32_t p1, uint32_t p2, uint32_t p3)
{
    if (!utf8_is_cont(p1)) { const uint32_t n = utf8_lead_need(p1); return n != kUtf8BadLead && n >= 1u; }
    if (!utf8_is_cont(p2)) { const uint32_t n = utf8_lead_need(p2); return n != kUtf8BadLead && n >= 2u; }
    return !utf8_is_cont(p3) && utf8_lead_need(p3) == 3u;
}

__host__ __device__ __forceinline__ uint32_t utf8_at(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t n1,
                                                     uint32_t n2, uint32_t n3)
{
    if (utf8_is_cont(b)) return utf8_cont_owned(p1, p2, p3) ? kUtf8Fine : kUtf8Invalid;
    return utf8_lead_class(b, n1, n2, n3);
}

// Position i < n of the string S(0 .. n - 1).
template <typename At>
__host__ __device__ __forceinline__ uint32_t utf8_at_by(At S, uint64_t n, uint64_t i)
{
    auto before = [&](uint64_t d) -> uint32_t { return i >= d ? S(i - d) : kUtf8Absent; };
    auto after = [&](uint64_t d) -> uint32_t { return n - i > d ? S(i + d) : kUtf8Absent; };
    return utf8_at(S(i), before(1), before(2), before(3), after(1), after(2), after(3));
}

// Is the message checked? carry: carry_in[m], 0 without carry_in.
__host__ __device__ __forceinline__ bool utf8_selected(uint32_t opcode, uint32_t msg_flags, uint64_t off, uint64_t size,
                                                       uint64_t payload_bytes, uint32_t carry)
{
    const bool text = opcode == 1u ||
                      (opcode == 0u && (msg_flags & CFWS_MESSAGE_HEADLESS) && (carry & CFWS_UTF8_CARRY_TEXT));
    return text && !(msg_flags & CFWS_MESSAGE_LOST_BYTES) && off + size >= off && off + size <= payload_bytes;
}

// The carried bytes in front of a checked message.
__host__ __device__ __forceinline__ uint32_t utf8_carried(uint32_t msg_flags, uint32_t carry)
{
    return (msg_flags & CFWS_MESSAGE_HEADLESS) ? (carry >> 24) & 3u : 0u;
}

// A checked message's row: S is the k carried bytes then the message's, n
// bytes in all; start == n when every position is fine, else the first one
// that is not, a truncated lead or not.
struct Utf8Row {
    uint64_t prefix;
    uint32_t carry, flags;
};

template <typename At>
__host__ __device__ __forceinline__ Utf8Row utf8_row(At S, uint64_t n, uint32_t k, uint32_t msg_flags, uint64_t start,
                                                     bool truncated)
{
    Utf8Row r = {(start > k ? start : k) - k, 0u, CFWS_UTF8_CHECKED};
    if (start == n) {
        r.flags |= CFWS_UTF8_VALID;
    } else if (truncated) {
        const uint32_t cnt = (uint32_t)(n - start);                  // 1..3
        for (uint32_t j = 0; j < cnt; ++j) r.carry |= (S(start + j) & 0xffu) << (8u * j);
        r.carry |= cnt << 24;
        r.flags |= CFWS_UTF8_TRUNCATED | ((msg_flags & CFWS_MESSAGE_OPEN) ? 0u : CFWS_UTF8_BAD);
    } else {
        r.flags |= CFWS_UTF8_INVALID | CFWS_UTF8_BAD;
    }
    return r;
}

#endif
