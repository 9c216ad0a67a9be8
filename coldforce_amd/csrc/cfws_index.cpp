// cfws_index.cpp -- receive-buffer frame indexing on the host (SURVEY §8 f#2).
//
// The frame walk of coldforce's receive loops, co_ws_server_on_tcp_receive_ready
// (src/ws/co_ws_server.c:107-169) and co_ws_client_on_tcp_receive_ready
// (src/ws/co_ws_client.c:200-270), without the per-frame payload copy: it
// only decodes the 2-14 header bytes of each frame (co_ws_frame.c:131-213)
// to find where the next one starts. The payloads are then copied + unmasked
// on the GPU by cfws_deserialize_* / cfws_pipeline_*. This is the host half
// of a receive loop whose bytes are in host memory (socket buffers); the
// device-resident form is cfws_index_frames_batch (cfws_ops.hip).
// Also the host form of the message and control tables of received frames
// (cfws_messages_from_frames; device form: cfws_messages.hip), and of the
// HTTP/2 stream grouping (cfws_h2_streams_from_frames; device form:
// cfws_h2streams.hip), and of the UTF-8 check of received text messages
// (cfws_utf8_check_messages; device form: cfws_utf8.hip).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cfws.h"
#include "cfws_rules.h"

namespace {

// Header at p of data[0, size) (size - p >= 2): COMPLETE and the frame's
// total length, or the code co_ws_frame_deserialize returns for it.
int32_t header_walk(const uint8_t* d, uint64_t size, uint64_t p, uint64_t max_payload,
                    uint64_t* frame_len)
{
    const uint64_t s = p;
    const uint32_t b0 = d[p], b1 = d[p + 1];
    p += 2;
    if ((b0 & 0x7fu) > 0x0f) return CFWS_ERROR_INVALID_FRAME;      // co_ws_frame.c:136-142
    uint64_t len = b1 & 0x7fu;
    if (len > 125) {                                                // :147-188
        const uint32_t ext = len == 126 ? 2u : 8u;
        if (size - p < ext) return CFWS_PARSE_MORE_DATA;
        len = 0;
        for (uint32_t i = 0; i < ext; ++i) len = (len << 8) | d[p + i];
        p += ext;
    }
    if (b1 & 0x80u) {                                               // :190-201
        if (size - p < 4) return CFWS_PARSE_MORE_DATA;
        p += 4;
    }
    if (size - p < len) return CFWS_PARSE_MORE_DATA;                // :203-206
    if (len > max_payload) return CFWS_ERROR_DATA_TOO_BIG;          // :208-213
    *frame_len = (p - s) + len;
    return CFWS_PARSE_COMPLETE;
}

}  // namespace

extern "C" {

size_t cfws_index_frames(const void* h_buf, uint64_t begin, uint64_t end, uint64_t max_payload,
                         uint64_t* starts, size_t max_starts, uint64_t* consumed, int32_t* stop)
{
    const uint8_t* d = static_cast<const uint8_t*>(h_buf);
    uint64_t p = begin;
    size_t k = 0;
    int32_t st = CFWS_PARSE_COMPLETE;
    while (end > p) {                                               // co_ws_server.c:107
        if (end - p < 2) { st = CFWS_PARSE_MORE_DATA; break; }      // :109-113
        uint64_t len = 0;
        st = header_walk(d, end, p, max_payload, &len);
        if (st != CFWS_PARSE_COMPLETE) break;                       // :144-166
        if (k == max_starts) { st = CFWS_INDEX_FULL; break; }       // resume at *consumed
        starts[k++] = p;
        p += len;                                                   // co_ws_frame.c:244
    }
    if (consumed) *consumed = p;
    if (stop) *stop = st;
    return k;
}

// The HTTP/2 receive loop's walk (co_http2_client.c:462-541) with the hop
// rule the device walk uses (h2_hop_by, cfws_rules.h). The rule asks for byte
// i only when i < end - p, so nothing outside [begin, end) is read.
size_t cfws_h2_index_frames(const void* h_buf, uint64_t begin, uint64_t end, uint32_t max_frame_size,
                            uint32_t select, uint32_t stream_id, uint64_t* starts,
                            cfws_h2_frame_info_t* info, size_t max_starts, uint64_t* consumed,
                            int32_t* stop)
{
    const uint8_t* d = static_cast<const uint8_t*>(h_buf);
    const uint32_t mfs = max_frame_size ? max_frame_size : CFWS_H2_DEFAULT_MAX_FRAME_SIZE;
    uint64_t p = begin;
    size_t k = 0;
    int32_t st = CFWS_H2_PARSE_COMPLETE;
    if (select > CFWS_H2_INDEX_DATA) {
        if (consumed) *consumed = begin;
        if (stop) *stop = CFWS_H2_PARSE_ERROR;
        return 0;
    }
    while (end > p) {                                               // co_http2_client.c:462
        const uint8_t* f = d + p;
        const H2Hop h = h2_hop_by([f](uint32_t i) -> uint32_t { return f[i]; }, end - p, mfs);
        st = h.status;
        if (st != CFWS_H2_PARSE_COMPLETE) break;                    // :475-536
        if (h2_selected(h, select, stream_id)) {
            if (k == max_starts) { st = CFWS_INDEX_FULL; break; }   // resume at *consumed
            starts[k] = p;
            if (info) info[k] = cfws_h2_frame_info_t{h.stream_id, h.length, h.advance, h.type, h.flags, 0};
            ++k;
        }
        p += h.advance;                                             // co_http2_frame.c:530
    }
    if (consumed) *consumed = p;
    if (stop) *stop = st;
    return k;
}

// The message rule (cfws_rules.h) as a walk: per connection, frames in index
// order, one message under construction while `open`. The device form
// (cfws_messages.hip) takes the same decisions from the same functions.
size_t cfws_messages_from_frames(const cfws_frame_desc_t* h_desc, const int32_t* h_status, size_t n_frames,
                                 const uint64_t* h_conn_first, size_t n_conns, cfws_message_t* msgs,
                                 size_t msg_capacity, uint64_t* conn_first_msg, uint32_t* control,
                                 size_t control_capacity, uint64_t* n_control)
{
    const size_t conns = h_conn_first ? n_conns : 1;
    auto bound = [&](size_t c) -> size_t {        // a value above n_frames is read as n_frames
        return h_conn_first[c] < n_frames ? (size_t)h_conn_first[c] : n_frames;
    };
    size_t m = 0;
    uint64_t nc = 0;
    for (size_t c = 0; c < conns; ++c) {
        const size_t lo = h_conn_first && c ? bound(c) : 0;
        const size_t hi = h_conn_first && c + 1 < conns ? bound(c + 1) : n_frames;
        if (conn_first_msg) conn_first_msg[c] = m;
        cfws_message_t cur = {};
        bool open = false, lost = false;
        auto end_message = [&](bool last_fin, bool followed) {
            cur.flags = (uint8_t)(cur.flags | message_end_flags(last_fin, followed, lost));
            if (m < msg_capacity) msgs[m] = cur;
            ++m;
        };
        for (size_t f = lo; f < hi; ++f) {
            const cfws_frame_desc_t& d = h_desc[f];
            const int32_t st = h_status ? h_status[f] : CFWS_PARSE_COMPLETE;
            const uint32_t cls = message_frame_class(st, d.opcode);
            if (cls == kMessageFrameIgnored) continue;
            if (cls == kMessageFrameControl) {
                if (nc < control_capacity) control[nc] = (uint32_t)f;
                ++nc;
                continue;
            }
            if (message_starts(d.opcode, open)) {
                if (open) end_message(false, true);
                cur = cfws_message_t{d.payload_off, 0, (uint32_t)f, 0, (uint32_t)c, d.opcode,
                                     (uint8_t)message_start_flags(d.opcode), 0};
                lost = false;
            }
            cur.payload_size += d.payload_size;
            ++cur.n_fragments;
            lost = lost || st == CFWS_ERROR_OUT_OF_MEMORY;
            open = d.fin == 0;
            if (!open) end_message(true, false);
        }
        if (open) end_message(false, false);
    }
    if (n_control) *n_control = nc;
    return m;
}

// The UTF-8 rule (cfws_rules.h) as a scalar walk: per checked message, the
// carried bytes then its own, position by position with the functions the
// kernel's lanes call (cfws_utf8.hip); runs of ASCII are stepped over eight
// bytes at a time and a well-formed lead's continuation bytes with it.
size_t cfws_utf8_check_messages(const void* h_payload, uint64_t payload_bytes, const cfws_message_t* h_msgs,
                                size_t n_msgs, const uint32_t* h_carry_in, cfws_utf8_result_t* result,
                                uint32_t* bad, size_t bad_capacity, uint64_t counts[2])
{
    const uint8_t* d = static_cast<const uint8_t*>(h_payload);
    uint64_t checked = 0, n_bad = 0;
    for (size_t m = 0; m < n_msgs; ++m) {
        const cfws_message_t& msg = h_msgs[m];
        const uint32_t cin = h_carry_in ? h_carry_in[m] : 0u;
        result[m] = cfws_utf8_result_t{};
        if (!utf8_selected(msg.opcode, msg.flags, msg.payload_off, msg.payload_size, payload_bytes, cin)) continue;
        const uint32_t k = utf8_carried(msg.flags, cin);
        const uint8_t* body = d + msg.payload_off;
        const uint64_t n = k + msg.payload_size;
        auto S = [&](uint64_t j) -> uint32_t { return j < k ? (cin >> (8u * j)) & 0xffu : body[j - k]; };
        uint64_t i = 0;
        uint32_t cls = kUtf8Fine;
        while (i < n) {
            if (i >= k) {
                uint64_t w;
                while (n - i >= 8 && (memcpy(&w, body + (i - k), 8), (w & 0x8080808080808080ull) == 0)) i += 8;
                if (i == n) break;
            }
            const uint32_t b = S(i);
            if (b < 0x80u) { ++i; continue; }
            cls = utf8_at_by(S, n, i);
            if (cls != kUtf8Fine) break;
            i += 1 + (utf8_is_cont(b) ? 0u : utf8_lead_need(b));
        }
        const Utf8Row r = utf8_row(S, n, k, msg.flags, i, cls == kUtf8Truncated);
        result[m] = cfws_utf8_result_t{r.prefix, r.carry, (uint8_t)r.flags, 0, 0};
        ++checked;
        if (r.flags & CFWS_UTF8_BAD) {
            if (n_bad < bad_capacity) bad[n_bad] = (uint32_t)m;
            ++n_bad;
        }
    }
    if (counts) { counts[0] = checked; counts[1] = n_bad; }
    return (size_t)n_bad;
}

// The stream rule (cfws_rules.h) as a sort and a walk: per connection the
// pooled records, stably sorted by stream id; every run in that order is a
// closed message or its stream's tail. Closed messages and their frames go
// out first, then the tails. The device form (cfws_h2streams.hip) takes the
// same decisions from the same functions.
size_t cfws_h2_streams_from_frames(const uint64_t* starts, const cfws_h2_frame_info_t* info, size_t n_frames,
                                   const uint64_t* conn_first, size_t n_conns, uint64_t* order,
                                   uint32_t* order_frame, cfws_h2_stream_msg_t* msgs, uint64_t* conn_first_msg,
                                   uint64_t* stream_first, uint64_t counts[5])
{
    const size_t conns = conn_first ? n_conns : 1;
    auto bound = [&](size_t c) -> size_t {        // a value above n_frames is read as n_frames
        return conn_first[c] < n_frames ? (size_t)conn_first[c] : n_frames;
    };
    struct Run {
        cfws_h2_stream_msg_t msg;
        size_t at;                                // its first frame in `sorted`
    };
    std::vector<uint32_t> sorted;                 // every connection's pooled records, grouped
    std::vector<Run> runs;
    std::vector<uint32_t> one;
    size_t n_closed = 0, closed_frames = 0;
    for (size_t c = 0; c < conns; ++c) {
        const size_t lo = conn_first && c ? bound(c) : 0;
        const size_t hi = conn_first && c + 1 < conns ? bound(c + 1) : n_frames;
        if (conn_first_msg) conn_first_msg[c] = n_closed;
        one.clear();
        for (size_t f = lo; f < hi; ++f)
            if (h2_stream_pooled(info[f].type, info[f].stream_id)) one.push_back((uint32_t)f);
        std::stable_sort(one.begin(), one.end(),
                         [&](uint32_t a, uint32_t b) { return info[a].stream_id < info[b].stream_id; });
        bool padded = false, stream_start = false;
        for (size_t r = 0; r < one.size(); ++r) {
            const cfws_h2_frame_info_t& i = info[one[r]];
            const bool same = r > 0 && info[one[r - 1]].stream_id == i.stream_id;
            if (h2_stream_starts(r == 0, same, r > 0 && h2_stream_closes(info[one[r - 1]].flags))) {
                runs.push_back(Run{cfws_h2_stream_msg_t{0, 0, 0, (uint32_t)c, i.stream_id, 0, 0, 0, 0},
                                   sorted.size() + r});
                padded = false;
                stream_start = !same;
            }
            cfws_h2_stream_msg_t& m = runs.back().msg;
            m.length_sum += i.length;
            ++m.n_data;
            m.end_frame = one[r];
            padded = padded || (i.flags & kH2FlagPadded) != 0;
            const bool last = r + 1 == one.size() || info[one[r + 1]].stream_id != i.stream_id;
            if (h2_stream_closes(i.flags) || last) {
                m.flags = (uint8_t)h2_stream_msg_flags(h2_stream_closes(i.flags), stream_start, padded);
                if (m.flags & CFWS_H2_STREAM_CLOSED) {
                    ++n_closed;
                    closed_frames += m.n_data;
                }
            }
        }
        sorted.insert(sorted.end(), one.begin(), one.end());
    }
    size_t at[2] = {0, n_closed}, frame_at[2] = {0, closed_frames}, n_streams = 0;
    for (Run& r : runs) {
        const int tail = (r.msg.flags & CFWS_H2_STREAM_CLOSED) ? 0 : 1;
        r.msg.first = (uint32_t)frame_at[tail];
        for (uint32_t k = 0; k < r.msg.n_data; ++k) {
            const uint32_t f = sorted[r.at + k];
            if (order) order[frame_at[tail] + k] = starts[f];
            if (order_frame) order_frame[frame_at[tail] + k] = f;
        }
        if (r.msg.flags & CFWS_H2_STREAM_FIRST) {
            if (stream_first) stream_first[n_streams] = at[0];
            ++n_streams;
        }
        if (msgs) msgs[at[tail]] = r.msg;
        ++at[tail];
        frame_at[tail] += r.msg.n_data;
    }
    if (counts) {
        counts[0] = n_closed;
        counts[1] = closed_frames;
        counts[2] = runs.size() - n_closed;
        counts[3] = sorted.size() - closed_frames;
        counts[4] = n_streams;
    }
    return n_closed;
}

}  // extern "C"
