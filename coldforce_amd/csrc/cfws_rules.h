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

#endif
