// chunks_test.cpp -- the host-memory pipeline's three chunk cuts
// (coldforce_amd/csrc/cfws_chunks.h) checked by the properties that define
// them uniquely, in a stand-alone host program for a build with
// -fsanitize=address,undefined (make build/chunks_test): every array a cut
// reads is a heap allocation of exactly its size, so a read one entry outside
// is a report. No GPU, no library: the header alone.
//
// For each batch, cutting from frame 0 on:
//   * the chunks tile [0, n) in order (each starts where the last ended);
//   * every chunk obeys each limit, evaluated here from the definitions and
//     not through the header's helpers;
//   * every chunk is maximal: frame j would break a limit, or j == n (HTTP/2
//     receive: no later point where no message is open fits either);
//   * a first frame (HTTP/2 receive: a message) over a limit gives the error
//     (fits == false), and the batch ends there.
// Fixed cases at chunk 4096 (the smallest a pipeline takes) sit exactly on,
// one under and one over each limit; then seeded random batches of at most
// 64 frames. A violated property prints to stderr and exits 1. stdout: one
// line per cut with what was seen (tests/test_pipeline_chunks.py reads it):
//   <cut> batches <n> chunks <n> multi <chunks of 2+ frames> errors <n>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cfws_chunks.h"

using namespace cfws_chunks;

static const uint64_t kChunk = 4096;

struct Seen {
    const char* cut;
    uint64_t batches, chunks, multi, errors;
};

#define REQUIRE(cond, ...)                                                   \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);       \
            fprintf(stderr, __VA_ARGS__);                                    \
            fprintf(stderr, "\n");                                           \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }
template <typename T, size_t N>
static T pick(const T (&a)[N]) { return a[below(N)]; }

// a heap copy of exactly v.size() entries (one entry, never read, for none)
template <typename T>
static T* exact(const std::vector<T>& v)
{
    T* p = static_cast<T*>(malloc((v.empty() ? 1 : v.size()) * sizeof(T)));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return v.empty() ? p + 1 : p;      // none: its end, so any read is outside
}
template <typename T>
static void release(T* p, size_t n) { free(n ? p : p - 1); }

// ---- send ------------------------------------------------------------------

struct SendCodec {
    uint64_t mfs;      // 0: WebSocket; else WS over HTTP/2 DATA frames of at most mfs
    FrameBytes bytes(const cfws_frame_desc_t& d) const { return mfs ? h2_frame_bytes(d, mfs) : ws_frame_bytes(d); }
};

// the limits of frames [i, j), from their definitions
struct SendSums {
    uint64_t lo, hi, wire, out;
    bool ok;
};
static SendSums send_sums(const std::vector<cfws_frame_desc_t>& d, size_t i, size_t j, size_t max_frames,
                          uint64_t mfs)
{
    SendSums s = {UINT64_MAX, 0, 0, 0, false};
    for (size_t k = i; k < j; ++k) {
        if (d[k].payload_off < s.lo) s.lo = d[k].payload_off;
        if (d[k].payload_off + d[k].payload_size > s.hi) s.hi = d[k].payload_off + d[k].payload_size;
        const uint64_t W = 2 + (d[k].payload_size > 65535 ? 8 : d[k].payload_size > 125 ? 2 : 0) + (d[k].mask ? 4 : 0) +
                           d[k].payload_size;
        s.wire += W;
        s.out += mfs ? W + 9 * (W <= mfs ? 1 : (W + mfs - 1) / mfs) : W;
    }
    s.lo -= s.lo % 16;
    s.ok = s.hi - s.lo <= kChunk && s.wire <= kChunk && s.out <= kChunk && j - i <= max_frames;
    return s;
}

// returns the chunks cut, or -1 for the error
static long check_send(const std::vector<cfws_frame_desc_t>& d, size_t max_frames, uint64_t mfs, Seen& seen)
{
    const size_t n = d.size();
    cfws_frame_desc_t* heap = exact(d);
    const SendCodec codec{mfs};
    long chunks = 0;
    ++seen.batches;
    for (size_t i = 0; i < n;) {
        const SendCut c = send_cut(heap, n, i, kChunk, max_frames, codec);
        if (!c.fits) {
            REQUIRE(!send_sums(d, i, i + 1, max_frames, mfs).ok, "error at frame %zu, which fits alone", i);
            ++seen.errors;
            release(heap, n);
            return -1;
        }
        REQUIRE(c.j > i && c.j <= n, "chunk [%zu, %zu) of %zu", i, c.j, n);
        const SendSums s = send_sums(d, i, c.j, max_frames, mfs);
        REQUIRE(s.ok, "chunk [%zu, %zu) breaks a limit: span %llu wire %llu out %llu", i, c.j,
                (unsigned long long)(s.hi - s.lo), (unsigned long long)s.wire, (unsigned long long)s.out);
        REQUIRE(c.src_lo == s.lo && c.src_hi == s.hi && c.wire == s.wire && c.out == s.out,
                "chunk [%zu, %zu): spans reported differ", i, c.j);
        REQUIRE(c.j == n || !send_sums(d, i, c.j + 1, max_frames, mfs).ok, "chunk [%zu, %zu) is not maximal", i, c.j);
        ++seen.chunks;
        seen.multi += c.j - i > 1;
        ++chunks;
        i = c.j;
    }
    release(heap, n);
    return chunks;
}

static cfws_frame_desc_t frame(uint64_t off, uint64_t size, bool mask)
{
    cfws_frame_desc_t f = {};
    f.payload_off = off;
    f.payload_size = size;
    f.mask = mask;
    f.fin = 1;
    f.opcode = 2;
    return f;
}

static void send_cases(Seen& ws, Seen& h2)
{
    // wire bytes exactly on / one under / one over the chunk (unmasked: 4 header bytes)
    REQUIRE(check_send({frame(0, 4092, false)}, 3, 0, ws) == 1, "4096 wire bytes fit");
    REQUIRE(check_send({frame(0, 4091, false)}, 3, 0, ws) == 1, "4095 wire bytes fit");
    REQUIRE(check_send({frame(0, 4093, false)}, 3, 0, ws) == -1, "4097 wire bytes do not");
    REQUIRE(check_send({frame(16, 4088, true)}, 1, 0, ws) == 1, "masked: 8 header bytes");
    REQUIRE(check_send({frame(16, 4089, true)}, 1, 0, ws) == -1, "masked, one over");
    // the source span counts from the 16-byte boundary below it
    REQUIRE(check_send({frame(15, 4081, false)}, 3, 0, ws) == 1, "span 15 + 4081 = 4096");
    REQUIRE(check_send({frame(15, 4082, false)}, 3, 0, ws) == -1, "span 4097, wire 4086");
    REQUIRE(check_send({frame(31, 1, false), frame(0, 0, false), frame(4095, 1, false)}, 3, 0, ws) == 1, "span 4096");
    REQUIRE(check_send({frame(31, 1, false), frame(0, 0, false), frame(4096, 1, false)}, 3, 0, ws) == 2, "span 4097");
    // payload_off jumps backwards past the chunk: a cut, not an error
    REQUIRE(check_send({frame(8191, 125, true), frame(15, 126, true), frame(8000, 0, false)}, 3, 0, ws) == 3, "jumps");
    // sums: 2 x 2048 wire bytes fit, one byte more does not; then the frame limit
    REQUIRE(check_send({frame(0, 2044, false), frame(0, 2044, false)}, 2, 0, ws) == 1, "2 x 2048");
    REQUIRE(check_send({frame(0, 2044, false), frame(0, 2045, false)}, 2, 0, ws) == 2, "2048 + 2049");
    REQUIRE(check_send({frame(0, 2044, false), frame(0, 2044, false)}, 1, 0, ws) == 2, "max_frames 1");
    REQUIRE(check_send({frame(0, 0, false), frame(0, 1, false), frame(0, 125, true), frame(0, 126, true)}, 3, 0, ws) == 2,
            "max_frames 3 of 4");
    REQUIRE(check_send({}, 3, 0, ws) == 0, "no frames");
    // HTTP/2: W + 9 * data_frames_of(W, mfs). mfs 16384: one DATA frame each
    REQUIRE(check_send({frame(0, 4083, false)}, 3, 16384, h2) == 1, "4087 + 9 = 4096");
    REQUIRE(check_send({frame(0, 4084, false)}, 3, 16384, h2) == -1, "4088 + 9");
    // mfs 16: W = 2620 is 164 DATA frames, 2620 + 1476 = 4096
    REQUIRE(check_send({frame(0, 2616, false)}, 3, 16, h2) == 1, "2620 wire bytes in 164 DATA frames");
    REQUIRE(check_send({frame(0, 2617, false)}, 3, 16, h2) == -1, "2621 wire bytes in 164 DATA frames");
    REQUIRE(check_send({frame(0, 0, false), frame(0, 0, false)}, 2, 16, h2) == 1, "empty frames: one DATA frame each");
    REQUIRE(check_send({frame(0, 1306, false), frame(0, 1306, false)}, 2, 16, h2) == 1, "2 x (1310 + 82 x 9) = 4096");
    REQUIRE(check_send({frame(0, 1306, false), frame(0, 1307, false)}, 2, 16, h2) == 2, "one byte more");
}

static void send_random(Seen& ws, Seen& h2, int batches)
{
    static const uint64_t sizes[] = {0, 0, 1, 1, 5, 125, 125, 126, 126, 127, 300, 700, 1306, 2044, 2616, 2617,
                                     4079, 4081, 4082, 4083, 4084, 4088, 4091, 4092, 4093, 5000};
    static const size_t frames[] = {1, 2, 3, 3, 64};
    static const uint64_t mfss[] = {0, 16, 16384};
    for (int b = 0; b < batches; ++b) {
        const size_t n = below(65);
        const bool small = below(3) != 0;           // mostly batches whose chunks take several frames
        std::vector<cfws_frame_desc_t> d;
        uint64_t off = below(10000);
        for (size_t k = 0; k < n; ++k) {
            const uint64_t sz = small ? pick(sizes) % 301 : pick(sizes);
            switch (below(4)) {
            case 0: off = below(20000); break;                   // anywhere, backwards too
            case 1: off = (off | 15); break;                     // off % 16 == 15
            default: break;                                      // contiguous
            }
            d.push_back(frame(off, sz, below(2)));
            off += sz;
        }
        const uint64_t mfs = pick(mfss);
        check_send(d, pick(frames), mfs, mfs ? h2 : ws);
    }
}

// ---- receive ---------------------------------------------------------------

// An index whose last frame ends where a walk stopped (cfws_pipeline_receive)
struct WalkedIndex {
    const uint64_t* starts;
    size_t n;
    uint64_t stop;
    bool has(size_t k) const { return k < n; }
    uint64_t at(size_t k) const { return starts[k]; }
    uint64_t last_end(uint64_t size) const { return stop < size ? stop : size; }
};

// staging need of frames [i, j): wire bytes from the 16-byte boundary below
// start i to the end of frame j - 1, plus align - 1 padding bytes per frame
static uint64_t need_of(const std::vector<uint64_t>& st, uint64_t size, uint64_t last_end, size_t i, size_t j,
                        uint32_t align)
{
    const uint64_t lo = st[i] < size ? st[i] : size;
    const uint64_t hi = j < st.size() ? (st[j] < size ? st[j] : size) : last_end;
    return hi - lo + lo % 16 + (j - i) * uint64_t(align - 1);
}

static long check_recv(const std::vector<uint64_t>& st, uint64_t size, uint64_t stop, size_t max_frames,
                       uint32_t align, Seen& seen)
{
    const size_t n = st.size();
    uint64_t* heap = exact(st);
    const uint64_t last_end = stop < size ? stop : size;
    long chunks = 0;
    ++seen.batches;
    for (size_t i = 0; i < n;) {
        RecvCut c;
        if (stop == UINT64_MAX) {
            ArrayIndex idx{heap, n};
            c = recv_cut(idx, size, i, kChunk, max_frames, align);
        } else {
            WalkedIndex idx{heap, n, stop};
            c = recv_cut(idx, size, i, kChunk, max_frames, align);
        }
        if (!c.fits) {
            REQUIRE(need_of(st, size, last_end, i, i + 1, align) > kChunk, "error at frame %zu, which fits alone", i);
            ++seen.errors;
            release(heap, n);
            return -1;
        }
        REQUIRE(c.j > i && c.j <= n, "chunk [%zu, %zu) of %zu", i, c.j, n);
        REQUIRE(need_of(st, size, last_end, i, c.j, align) <= kChunk && c.j - i <= max_frames,
                "chunk [%zu, %zu) breaks a limit", i, c.j);
        const uint64_t lo = st[i] < size ? st[i] : size;
        REQUIRE(c.wire_lo == lo - lo % 16 && c.hi - c.wire_lo + (c.j - i) * uint64_t(align - 1) ==
                                                 need_of(st, size, last_end, i, c.j, align),
                "chunk [%zu, %zu): spans reported differ", i, c.j);
        REQUIRE(c.j == n || c.j - i == max_frames || need_of(st, size, last_end, i, c.j + 1, align) > kChunk,
                "chunk [%zu, %zu) is not maximal", i, c.j);
        ++seen.chunks;
        seen.multi += c.j - i > 1;
        ++chunks;
        i = c.j;
    }
    release(heap, n);
    return chunks;
}

static std::vector<uint64_t> starts_of(uint64_t first, const std::vector<uint64_t>& sizes)
{
    std::vector<uint64_t> st;
    for (uint64_t s : sizes) {
        st.push_back(first);
        first += s;
    }
    return st;
}

static void recv_cases(Seen& seen)
{
    const uint64_t whole = UINT64_MAX;
    REQUIRE(check_recv(starts_of(0, {4096}), 4096, whole, 3, 1, seen) == 1, "a frame of the chunk's size");
    REQUIRE(check_recv(starts_of(0, {4097}), 4097, whole, 3, 1, seen) == -1, "one byte more");
    REQUIRE(check_recv(starts_of(15, {4081}), 4096, whole, 3, 1, seen) == 1, "15 + 4081 from the boundary below");
    REQUIRE(check_recv(starts_of(15, {4082}), 4097, whole, 3, 1, seen) == -1, "15 + 4082");
    REQUIRE(check_recv(starts_of(0, {4081}), 4081, whole, 3, 16, seen) == 1, "4081 + 15 padding bytes");
    REQUIRE(check_recv(starts_of(0, {4082}), 4082, whole, 3, 16, seen) == -1, "4082 + 15");
    REQUIRE(check_recv(starts_of(0, {1}), 1, whole, 3, 4096, seen) == 1, "1 + 4095 padding bytes");
    REQUIRE(check_recv(starts_of(0, {2}), 2, whole, 3, 4096, seen) == -1, "2 + 4095");
    REQUIRE(check_recv(starts_of(0, {2, 125, 126, 2}), 255, whole, 3, 1, seen) == 2, "max_frames 3 of 4");
    REQUIRE(check_recv(starts_of(0, {2, 125, 126, 2}), 255, whole, 1, 16, seen) == 4, "max_frames 1");
    REQUIRE(check_recv(starts_of(0, {2048, 2048, 1}), 4097, whole, 3, 1, seen) == 2, "2 x 2048, then the rest");
    REQUIRE(check_recv(starts_of(0, {2041, 2025, 3000}), 7066, whole, 2, 16, seen) == 2, "4066 + 2 x 15 = 4096");
    REQUIRE(check_recv(starts_of(0, {2041, 2026, 3000}), 7067, whole, 2, 16, seen) == 3, "4067 + 2 x 15");
    // starts at and past the buffer's end (truncated tails) are clamped to it
    REQUIRE(check_recv({0, 100, 199, 200, 5000}, 200, whole, 64, 1, seen) == 1, "clamped starts");
    // a walk's stop ends the last frame: the bytes after it are not counted
    REQUIRE(check_recv(starts_of(0, {4000, 96}), 9000, 4096, 2, 1, seen) == 1, "ends at the walk's stop");
    REQUIRE(check_recv(starts_of(0, {4000, 97}), 9000, 4097, 2, 1, seen) == 2, "one byte more");
    REQUIRE(check_recv({}, 0, whole, 3, 16, seen) == 0, "no frames");
}

static void recv_random(Seen& seen, int batches)
{
    static const uint64_t sizes[] = {2, 2, 3, 6, 8, 127, 131, 134, 700, 1365, 2040, 2041, 2048, 4080, 4081, 4082,
                                     4096, 4097};
    static const size_t frames[] = {1, 2, 3, 3, 64};
    static const uint32_t aligns[] = {1, 1, 16, 16, 4096};
    for (int b = 0; b < batches; ++b) {
        const size_t n = below(65);
        const bool small = below(3) != 0;
        std::vector<uint64_t> sz;
        for (size_t k = 0; k < n; ++k) sz.push_back(small ? 2 + pick(sizes) % 140 : pick(sizes));
        const std::vector<uint64_t> st = starts_of(below(4) ? below(64) : 15, sz);
        uint64_t end = n ? st.back() + sz.back() : 0;
        uint64_t size = end, stop = UINT64_MAX;
        switch (below(4)) {
        case 0: size = end - below(end + 1) / 4; break;            // truncated: late starts clamp
        case 1: size = end + below(5000); stop = end; break;       // bytes after the walk's stop
        default: break;
        }
        check_recv(st, size, stop, pick(frames), pick(aligns), seen);
    }
}

// ---- HTTP/2 receive --------------------------------------------------------

struct H2Buf {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> starts;
    // type 0: DATA. flags: 0x1 END_STREAM, 0x8 PADDED (one pad length byte + pad bytes inside len)
    void add(uint32_t len, uint8_t type, uint8_t flags, uint8_t pad = 0)
    {
        starts.push_back(bytes.size());
        const uint8_t h[9] = {uint8_t(len >> 16), uint8_t(len >> 8), uint8_t(len), type, flags, 0, 0, 0, 1};
        bytes.insert(bytes.end(), h, h + 9);
        for (uint32_t k = 0; k < len; ++k) bytes.push_back((flags & 0x8) && k == 0 ? pad : uint8_t(rnd()));
    }
    // a length field over any max_frame_size, with `body` bytes behind it: PARSE_ERROR, not pooled
    void add_corrupt(uint32_t body, uint8_t flags)
    {
        add(body, 0, flags);
        bytes[starts.back()] = 0xFF;
    }
};

// what frames [i, j) pool, and the bytes of a message still open after them
struct Pool {
    uint64_t pooled, open;
};
static Pool pool_of(const H2Buf& b, uint64_t size, size_t i, size_t j, uint64_t mfs)
{
    Pool p = {0, 0};
    for (size_t k = i; k < j; ++k) {
        const H2Frame f = h2_frame_at(b.bytes.data(), size, b.starts[k], mfs);
        if (f.status != CFWS_H2_PARSE_COMPLETE) continue;
        p.pooled += f.payload_size;
        p.open = f.end_stream ? 0 : p.open + f.payload_size;
    }
    return p;
}

static long check_h2_recv(const H2Buf& b, size_t max_frames, uint32_t align, uint64_t mfs, Seen& seen)
{
    const size_t n = b.starts.size();
    const uint64_t size = b.bytes.size();
    uint64_t* heap = exact(b.starts);
    uint8_t* h2 = exact(b.bytes);
    ArrayIndex idx{heap, n};
    // may frames [i, j) be a chunk? within the limits, and no message open or the stream's tail
    auto allowed = [&](size_t i, size_t j) {
        return need_of(b.starts, size, size, i, j, align) <= kChunk && j - i <= max_frames &&
               (j == n || pool_of(b, size, i, j, mfs).open == 0);
    };
    long chunks = 0;
    ++seen.batches;
    for (size_t i = 0; i < n;) {
        const RecvCut c = h2_recv_cut(idx, h2, size, i, kChunk, max_frames, align, mfs);
        // the limits only grow with j: the first j over one ends the search
        size_t last = i;
        for (size_t j = i + 1; j <= n && j - i <= max_frames && need_of(b.starts, size, size, i, j, align) <= kChunk; ++j)
            if (allowed(i, j)) last = j;
        if (!c.fits) {
            REQUIRE(last == i, "error at frame %zu, where [%zu, %zu) is a chunk", i, i, last);
            ++seen.errors;
            release(heap, n);
            release(h2, size);
            return -1;
        }
        REQUIRE(c.j > i && c.j <= n && allowed(i, c.j), "chunk [%zu, %zu) of %zu breaks a limit or a message", i, c.j, n);
        REQUIRE(c.j == last, "chunk [%zu, %zu) is not maximal: [%zu, %zu) fits", i, c.j, i, last);
        const uint64_t lo = b.starts[i];
        REQUIRE(c.wire_lo == lo - lo % 16 && c.hi == (c.j < n ? b.starts[c.j] : size) &&
                    c.pooled == pool_of(b, size, i, c.j, mfs).pooled,
                "chunk [%zu, %zu): spans or pooled bytes reported differ", i, c.j);
        ++seen.chunks;
        seen.multi += c.j - i > 1;
        ++chunks;
        i = c.j;
    }
    release(heap, n);
    release(h2, size);
    return chunks;
}

static void h2_recv_cases(Seen& seen)
{
    {   // a message that fills the chunk exactly: 4 DATA frames, 4 x (9 + 1015) = 4096
        H2Buf b;
        for (int k = 0; k < 4; ++k) b.add(1015, 0, k == 3);
        REQUIRE(check_h2_recv(b, 64, 1, 16384, seen) == 1, "a message of the chunk's size");
    }
    {   // one byte too long: no point inside it where no message is open
        H2Buf b;
        for (int k = 0; k < 4; ++k) b.add(k ? 1015 : 1016, 0, k == 3);
        b.add(5, 0, 1);
        REQUIRE(check_h2_recv(b, 64, 1, 16384, seen) == -1, "a message one byte too long");
    }
    {   // more DATA frames than max_frames
        H2Buf b;
        for (int k = 0; k < 3; ++k) b.add(10, 0, k == 2);
        REQUIRE(check_h2_recv(b, 3, 16, 16384, seen) == 1, "3 frames, max_frames 3");
        REQUIRE(check_h2_recv(b, 2, 16, 16384, seen) == -1, "3 frames, max_frames 2");
    }
    {   // cuts fall between messages only; the second chunk is the unterminated tail
        H2Buf b;
        b.add(2000, 0, 1);
        b.add(1000, 0, 0);
        b.add(1000, 0, 1);
        b.add(1000, 0, 0);
        b.add(500, 0, 0);
        REQUIRE(check_h2_recv(b, 64, 1, 16384, seen) == 2, "message | message + tail... cut where closed");
    }
    {   // a non-DATA frame between a message's DATA frames pools nothing and closes nothing
        H2Buf b;
        b.add(1500, 0, 0);
        b.add(12, 4, 0);
        b.add(1500, 0, 1);
        b.add(1500, 0, 1);
        REQUIRE(check_h2_recv(b, 3, 1, 16384, seen) == 2, "DATA, SETTINGS, DATA | DATA");
        REQUIRE(check_h2_recv(b, 2, 1, 16384, seen) == -1, "the message is 3 frames with the SETTINGS frame");
    }
    {   // a corrupt length is not pooled: its END_STREAM does not close, its bytes do not open
        H2Buf b;
        b.add(100, 0, 0);
        b.add_corrupt(100, 1);
        b.add(100, 0, 1);
        b.add_corrupt(100, 0);
        b.add(100, 0, 1);
        REQUIRE(check_h2_recv(b, 2, 1, 16384, seen) == -1, "open across the corrupt END_STREAM frame");
        REQUIRE(check_h2_recv(b, 3, 1, 16384, seen) == 2, "closed after 3; the corrupt frame opens nothing");
    }
    {   // mfs 16: a 17-byte frame is over max_frame_size (PARSE_ERROR), 16 is not; padding is not pooled
        H2Buf b;
        b.add(16, 0, 0);
        b.add(17, 0, 1);
        b.add(16, 0x0, 0x9, 3);       // END_STREAM | PADDED: 1 + 12 + 3
        b.add(16, 0, 0);
        REQUIRE(check_h2_recv(b, 2, 16, 16, seen) == -1, "the 17-byte END_STREAM frame does not close");
        REQUIRE(check_h2_recv(b, 3, 16, 16, seen) == 2, "three frames, then the tail");
        REQUIRE(check_h2_recv(b, 2, 16, 16384, seen) == 2, "mfs 16384: the 17-byte frame closes");
    }
    {
        H2Buf b;
        REQUIRE(check_h2_recv(b, 3, 16, 16384, seen) == 0, "no frames");
    }
}

static void h2_recv_random(Seen& seen, int batches)
{
    static const size_t frames[] = {1, 2, 3, 3, 64};
    static const uint32_t aligns[] = {1, 1, 1, 16, 16, 16, 4096};
    static const uint32_t lens[] = {0, 1, 5, 16, 16, 17, 100, 126, 700, 1015, 1016, 2000, 4087, 4088};
    for (int b = 0; b < batches; ++b) {
        const size_t n = below(65);
        const uint64_t mfs = below(2) ? 16 : 16384;
        const bool small = below(3) != 0;
        H2Buf buf;
        for (size_t k = 0; k < n; ++k) {
            const uint32_t len = small ? pick(lens) % 18 : pick(lens);
            const uint8_t end = below(3) != 0;
            switch (below(12)) {
            case 0: buf.add(len % 40, uint8_t(1 + below(9)), end); break;               // a non-DATA frame
            case 1: buf.add_corrupt(len % 40, end); break;
            case 2: buf.add(len ? len : 1, 0, uint8_t(0x8 | end), uint8_t(below((len < 200 ? len : 200) + 2))); break;   // PADDED, at times past the frame
            default: buf.add(len, 0, end); break;
            }
        }
        if (below(4) == 0 && !buf.bytes.empty()) buf.bytes.resize(buf.bytes.size() - below(9));   // a cut last frame
        check_h2_recv(buf, pick(frames), pick(aligns), mfs, seen);
    }
}

int main()
{
    Seen ws = {"send", 0, 0, 0, 0}, h2s = {"h2_send", 0, 0, 0, 0}, rx = {"recv", 0, 0, 0, 0},
         h2r = {"h2_recv", 0, 0, 0, 0};
    send_cases(ws, h2s);
    recv_cases(rx);
    h2_recv_cases(h2r);
    send_random(ws, h2s, 6000);
    recv_random(rx, 3000);
    h2_recv_random(h2r, 3000);
    for (const Seen* s : {&ws, &h2s, &rx, &h2r})
        printf("%s batches %llu chunks %llu multi %llu errors %llu\n", s->cut, (unsigned long long)s->batches,
               (unsigned long long)s->chunks, (unsigned long long)s->multi, (unsigned long long)s->errors);
    return 0;
}
