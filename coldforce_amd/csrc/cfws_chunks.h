// cfws_chunks.h -- how the host-memory pipeline (cfws_pipeline.cpp) cuts a
// batch into chunks: three greedy cuts over host arrays, each written once.
// Host only, no HIP types: tests/native/chunks_test.cpp checks them in a
// stand-alone program by the properties that define them (the chunks tile the
// batch, each obeys every limit, each is maximal).
//
// A cut takes the chunk size (a slot's staging bytes per direction),
// max_frames (>= 1, a slot's descriptor staging) and the first frame i, and
// returns j (the chunk is frames [i, j), j > i), the spans its caller stages,
// and `fits`: false when even the smallest chunk the cut may take breaks a
// limit, the caller's error.
#ifndef CFWS_CHUNKS_H
#define CFWS_CHUNKS_H

#include <stddef.h>
#include <stdint.h>

#include "cfws.h"
#include "cfws_rules.h"

namespace cfws_chunks {

// Staged spans start on a 16-byte boundary of the host buffer, so the device
// copy keeps the source's alignment.
inline uint64_t down16(uint64_t x) { return x & ~uint64_t(15); }

// ---- send --------------------------------------------------------------

// What one frame adds to each byte sum a send chunk must hold: its WS wire
// bytes, and the bytes of the output stream it becomes.
struct FrameBytes {
    uint64_t wire, out;
};

// WebSocket: the output is the wire.
inline FrameBytes ws_frame_bytes(const cfws_frame_desc_t& d)
{
    const uint64_t W = header_size_of(d.payload_size, d.mask != 0) + d.payload_size;
    return {W, W};
}

// WS over HTTP/2: the wire (the two-pass form's scratch) cut into DATA frames
// of at most mfs bytes, 9 header bytes each.
inline FrameBytes h2_frame_bytes(const cfws_frame_desc_t& d, uint64_t mfs)
{
    const uint64_t W = header_size_of(d.payload_size, d.mask != 0) + d.payload_size;
    return {W, W + 9 * data_frames_of(W, mfs)};
}

struct SendCut {
    size_t j;
    uint64_t src_lo, src_hi;   // payload arena bytes staged: [down16(min payload_off), max end)
    uint64_t wire, out;        // the chunk's byte sums
    bool fits;                 // false: frame i alone exceeds a limit
};

// Frames [i, j): the source span (payload_off may jump either way), the wire
// bytes and the output bytes each within `chunk`, at most max_frames frames.
// codec.bytes(desc) gives a frame's FrameBytes. The first frame is always
// taken.
template <typename Codec>
SendCut send_cut(const cfws_frame_desc_t* desc, size_t n, size_t i, uint64_t chunk, size_t max_frames,
                 const Codec& codec)
{
    uint64_t lo = desc[i].payload_off, hi = lo + desc[i].payload_size, wire = 0, out = 0;
    size_t j = i;
    while (j < n && j - i < max_frames) {
        const uint64_t a = lo < desc[j].payload_off ? lo : desc[j].payload_off;
        const uint64_t e = desc[j].payload_off + desc[j].payload_size, b = hi > e ? hi : e;
        const FrameBytes f = codec.bytes(desc[j]);
        if (j > i && (b - down16(a) > chunk || wire + f.wire > chunk || out + f.out > chunk)) break;
        lo = a;
        hi = b;
        wire += f.wire;
        out += f.out;
        ++j;
    }
    const uint64_t src_lo = down16(lo);
    return {j, src_lo, hi, wire, out, !(hi - src_lo > chunk || wire > chunk || out > chunk)};
}

// ---- receive -----------------------------------------------------------
//
// The frame starts come through an index with
//   bool has(size_t k)               does start k exist?
//   uint64_t at(size_t k)            start k (has(k) was true)
//   uint64_t last_end(uint64_t size) where the last frame's bytes end
// (cfws_pipeline.cpp's StartSource; ArrayIndex below for a plain array).
// Starts increase, and a frame's bytes end at the next frame's start.

struct ArrayIndex {
    const uint64_t* starts;
    size_t n;
    bool has(size_t k) const { return k < n; }
    uint64_t at(size_t k) const { return starts[k]; }
    uint64_t last_end(uint64_t size) const { return size; }
};

template <typename Index>
uint64_t start_of(Index& idx, size_t k, uint64_t size)
{
    const uint64_t s = idx.at(k);
    return s < size ? s : size;
}

template <typename Index>
uint64_t end_of(Index& idx, size_t k, uint64_t size)
{
    return idx.has(k + 1) ? start_of(idx, k + 1, size) : idx.last_end(size);
}

// A receive chunk's staging need: its wire bytes from the 16-byte boundary
// below its first start, plus the worst-case alignment padding of its
// payloads in the output.
inline uint64_t recv_need(uint64_t wire_lo, uint64_t hi, size_t frames, uint32_t align)
{
    return hi - wire_lo + frames * uint64_t(align - 1);
}

struct RecvCut {
    size_t j;
    uint64_t wire_lo, hi;      // buffer bytes staged: [down16(start i), end of frame j - 1)
    uint64_t pooled;           // HTTP/2: DATA payload bytes the chunk's frames pool
    bool fits;                 // false: see each cut
};

// Frames [i, j): recv_need within `chunk`, at most max_frames frames. The
// first frame is always taken; fits is false when it alone needs more.
template <typename Index>
RecvCut recv_cut(Index& idx, uint64_t size, size_t i, uint64_t chunk, size_t max_frames, uint32_t align)
{
    const uint64_t wire_lo = down16(start_of(idx, i, size));
    size_t j = i + 1;
    while (idx.has(j) && j - i < max_frames && recv_need(wire_lo, end_of(idx, j, size), j + 1 - i, align) <= chunk)
        ++j;
    const uint64_t hi = end_of(idx, j - 1, size);
    return {j, wire_lo, hi, 0, recv_need(wire_lo, hi, j - i, align) <= chunk};
}

// HTTP/2: the receive cut's limits, ending at the last j where no message is
// open, so every message is decoded whole. Open is decided as the device
// decides it (h2_frame_at): only a COMPLETE DATA frame pools its payload, and
// END_STREAM closes the message. The stream's tail (j reaches the last
// start) is taken even with a message open. fits is false when no such j
// exists: a message spans more bytes or frames than a chunk holds.
template <typename Index>
RecvCut h2_recv_cut(Index& idx, const uint8_t* h2, uint64_t size, size_t i, uint64_t chunk, size_t max_frames,
                    uint32_t align, uint64_t mfs)
{
    const uint64_t wire_lo = down16(start_of(idx, i, size));
    uint64_t open = 0, pooled = 0, best_pooled = 0;
    size_t j = i, best = i;
    while (idx.has(j) && j - i < max_frames && recv_need(wire_lo, end_of(idx, j, size), j + 1 - i, align) <= chunk) {
        const H2Frame fr = h2_frame_at(h2, size, idx.at(j), mfs);
        if (fr.status == CFWS_H2_PARSE_COMPLETE) {
            pooled += fr.payload_size;
            open = fr.end_stream ? 0 : open + fr.payload_size;
        }
        ++j;
        if (open == 0 || !idx.has(j)) {
            best = j;
            best_pooled = pooled;
        }
    }
    if (best == i) return {i, wire_lo, wire_lo, 0, false};
    return {best, wire_lo, end_of(idx, best - 1, size), best_pooled, true};
}

}  // namespace cfws_chunks

#endif
