/*
 * cfws.h -- MI355X batch WebSocket frame codec: C ABI over device arenas.
 *
 * This is the batch entry point that sits beside the drop-in per-frame API
 * (include/cfws_co_ws_frame.h). It covers the hot path of coldforce's
 * src/ws/co_ws_frame.c for many independent frames at once:
 *
 *   cfws_serialize_*   = co_ws_frame_serialize   (co_ws_frame.c:21-119)
 *                        for every frame of a batch: header encode + 4-byte
 *                        key XOR mask, frames packed back to back in a wire
 *                        arena exactly as sequential appends to one
 *                        co_byte_array_t would lay them out.
 *   cfws_deserialize_* = co_ws_frame_deserialize (co_ws_frame.c:121-247)
 *                        at each given frame start of a wire arena (as the
 *                        receive loops call it, co_ws_server.c:107-169):
 *                        header decode, MORE_DATA / INVALID_FRAME /
 *                        DATA_TOO_BIG decisions, copy + XOR unmask of every
 *                        COMPLETE payload into a payload arena.
 *
 * Every pointer argument named d_* is device memory (hipMalloc); `stream` is
 * a hipStream_t (NULL = default stream). Nothing here synchronises: results
 * are valid once the stream has reached the end of the call. All arenas
 * must be 16-byte aligned. The library needs a gfx950 device; with none it
 * returns CFWS_ERROR_NO_DEVICE (there is no CPU fallback).
 */
#ifndef CFWS_H
#define CFWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes of the batch API. */
#define CFWS_OK                       0
#define CFWS_ERROR_INVALID_ARGUMENT  (-1)
#define CFWS_ERROR_WORKSPACE         (-2)
#define CFWS_ERROR_HIP               (-3)
#define CFWS_ERROR_NO_DEVICE         (-4)

/* Per-frame status codes written by deserialize: the reference's own values
 * (inc/coldforce/ws/co_ws.h:25-39). */
#define CFWS_PARSE_COMPLETE           0
#define CFWS_PARSE_MORE_DATA          1
#define CFWS_ERROR_INVALID_FRAME     (-7001)
#define CFWS_ERROR_DATA_TOO_BIG      (-7005)
#define CFWS_ERROR_OUT_OF_MEMORY     (-7006)

/* Default max receive payload, co_ws_config.h:15. */
#define CFWS_DEFAULT_MAX_RECEIVE_PAYLOAD_SIZE ((uint64_t)32 * 1024 * 1024)

/*
 * One frame of a batch (32 bytes, device resident, array-of-structs).
 *   serialize:   in  payload_off, payload_size, mask_key, fin, opcode, mask
 *                out wire_off, header_size
 *   deserialize: in  wire_off (the frame start, from the caller's index)
 *                out everything else, as far as the header was parsed
 * mask_key holds the 4 key bytes in wire order: byte j = (mask_key >> 8j).
 * opcode is written to the wire verbatim, OR 0x80 when fin (co_ws_frame.c
 * :34-39); deserialize reports opcode = b0 & 0x7f (co_ws_frame.c:136-137).
 */
typedef struct cfws_frame_desc {
    uint64_t payload_off;
    uint64_t wire_off;
    uint64_t payload_size;
    uint32_t mask_key;
    uint8_t  fin;
    uint8_t  opcode;
    uint8_t  mask;
    uint8_t  header_size;
} cfws_frame_desc_t;

/* Library / device check: CFWS_OK when the calling thread's current HIP
 * device is a gfx950. Every visible device is probed once per process
 * (thread-safe); cfws_init_device checks one device by ordinal. */
int cfws_init(void);
int cfws_init_device(int device);
const char* cfws_last_error(void);
const char* cfws_version(void);

/* Bytes of device workspace a plan+execute over n_frames frames producing
 * at most out_capacity output bytes needs. */
size_t cfws_workspace_size(size_t n_frames, uint64_t out_capacity);

/* ---- serialize (client mask / server plain) ------------------------------
 * plan:    header sizes, wire offsets (prefix sum), tile map, and
 *          *d_wire_total = total wire bytes (not clamped to capacity).
 * execute: writes headers + (masked) payloads; bytes past wire_capacity are
 *          not written (check *d_wire_total <= wire_capacity).
 * The workspace carries the plan from plan to execute. */
int cfws_serialize_plan(cfws_frame_desc_t* d_desc, size_t n_frames,
                        uint64_t wire_capacity, uint64_t* d_wire_total,
                        void* d_workspace, size_t workspace_size, void* stream);
int cfws_serialize_execute(const void* d_payload, const cfws_frame_desc_t* d_desc,
                           size_t n_frames, void* d_wire, uint64_t wire_capacity,
                           const void* d_workspace, void* stream);
int cfws_serialize_batch(const void* d_payload, cfws_frame_desc_t* d_desc,
                         size_t n_frames, void* d_wire, uint64_t wire_capacity,
                         uint64_t* d_wire_total, void* d_workspace,
                         size_t workspace_size, void* stream);

/* ---- serialize a uniform batch (compact input) ----------------------------
 * Every frame has the same payload_size, fin, opcode and mask: n sequential
 * co_ws_frame_serialize calls (co_ws_frame.c:21-119) appending fixed-size
 * messages to one co_byte_array, with no descriptor table and no plan.
 * Frame i's payload is d_payload[i * payload_size, (i + 1) * payload_size)
 * and its key d_keys[i] (wire order, as cfws_frame_desc_t.mask_key; NULL
 * allowed when mask == 0); its frame is d_wire[i * W, (i + 1) * W), W =
 * header size (2..14, co_ws_frame.c:34-91) + payload_size. One launch, no
 * workspace; the bytes are those cfws_serialize_batch writes for the same
 * frames. Wire bytes at or past wire_capacity are not written;
 * *d_wire_total (may be NULL) = n * W. payload_size <= 2^30, n * W < 2^40. */
int cfws_serialize_uniform(const void* d_payload, const uint32_t* d_keys, size_t n_frames,
                           uint64_t payload_size, uint8_t fin, uint8_t opcode, uint8_t mask,
                           void* d_wire, uint64_t wire_capacity, uint64_t* d_wire_total,
                           void* stream);

/* ---- deserialize (server unmask / client plain) --------------------------
 * plan:    parses the header at each d_frame_index[i] against wire_size,
 *          writes d_desc[i] and d_status[i] (reference codes) and lays the
 *          COMPLETE payloads out:
 *            flags = 0: payload_off = exclusive prefix sum of
 *              round_up(payload_size, align) (align a power of two, 1..4096);
 *            flags = CFWS_DESERIALIZE_REASSEMBLE: data frames (opcode < 8)
 *              packed back to back in stream order, so the fragments of every
 *              message (TEXT/BINARY then CONTINUATION..., co_ws_frame.h:28-30)
 *              are contiguous; control frames (opcode 8-15) packed after all
 *              data bytes; align is ignored.
 *          A COMPLETE frame with a non-empty payload that does not fit
 *          payload_capacity gets CFWS_ERROR_OUT_OF_MEMORY (layout unchanged).
 *          *d_payload_total = min(sum, capacity).
 * execute: copies + unmasks every COMPLETE payload; bytes of the layout not
 *          covered by a payload (alignment padding, OOM frames) are zero.
 *          `flags` must be the plan's. */
#define CFWS_DESERIALIZE_REASSEMBLE 1u

int cfws_deserialize_plan(const void* d_wire, uint64_t wire_size,
                          const uint64_t* d_frame_index, size_t n_frames,
                          uint64_t max_payload, uint32_t align, uint32_t flags,
                          cfws_frame_desc_t* d_desc, int32_t* d_status,
                          uint64_t payload_capacity, uint64_t* d_payload_total,
                          void* d_workspace, size_t workspace_size, void* stream);
int cfws_deserialize_execute(const void* d_wire, const cfws_frame_desc_t* d_desc,
                             const int32_t* d_status, size_t n_frames, uint32_t flags,
                             void* d_payload, uint64_t payload_capacity,
                             const void* d_workspace, void* stream);
int cfws_deserialize_batch(const void* d_wire, uint64_t wire_size,
                           const uint64_t* d_frame_index, size_t n_frames,
                           uint64_t max_payload, uint32_t align, uint32_t flags,
                           cfws_frame_desc_t* d_desc, int32_t* d_status,
                           void* d_payload, uint64_t payload_capacity,
                           uint64_t* d_payload_total, void* d_workspace,
                           size_t workspace_size, void* stream);

/* ---- deserialize into fixed payload slots --------------------------------
 * The batch receive with frame i's payload at payload_off = i * slot_bytes
 * (slot_bytes a multiple of 16 in [16, 2^31]): the slab form of the
 * reference's one allocation per frame (co_ws_frame_deserialize,
 * src/ws/co_ws_frame.c:216-223). One launch, no workspace: no payload offset
 * depends on another frame, so each wire line is read once.
 *   d_desc[i], d_status[i]: as cfws_deserialize_plan (flags = 0), with the
 *     slot rule in place of the packing: a COMPLETE frame whose non-empty
 *     payload is longer than slot_bytes, or ends past payload_capacity, gets
 *     CFWS_ERROR_OUT_OF_MEMORY.
 *   slot i of a COMPLETE frame: the unmasked payload, then zeros up to the
 *     next 16-byte boundary (cut at the capacity); the rest of every slot,
 *     and the slots of all other frames, are not written.
 *   *d_payload_total (may be NULL) = min(n_frames * slot_bytes, capacity).
 * Frames of the same wire may be indexed in any order, overlapping or not. */
int cfws_deserialize_slots(const void* d_wire, uint64_t wire_size,
                           const uint64_t* d_frame_index, size_t n_frames,
                           uint64_t max_payload, uint64_t slot_bytes,
                           cfws_frame_desc_t* d_desc, int32_t* d_status,
                           void* d_payload, uint64_t payload_capacity,
                           uint64_t* d_payload_total, void* stream);

/* ---- compact per-frame output of the slot / scatter receives --------------
 * What the reference's frame object carries (co_ws_frame_header_t:
 * fin, opcode, payload_size, co_ws_frame.h:36-49) plus the status, in 8
 * bytes instead of the 36 of a descriptor + status (the payload offset is
 * the slot, or the caller's, and the key and header size are consumed by
 * the unmask). payload_size is the parsed length, UINT32_MAX when it does
 * not fit 32 bits (never for a COMPLETE frame: its payload fits its slot,
 * <= 2^31); status is the int32 code cast to 16 bits (every code fits). */
typedef struct cfws_frame_info {
    uint32_t payload_size;
    uint8_t  fin;
    uint8_t  opcode;
    int16_t  status;
} cfws_frame_info_t;

/* cfws_deserialize_slots / cfws_deserialize_scatter with d_info[i] (8-byte
 * aligned; CFWS_ERROR_INVALID_ARGUMENT otherwise) in place of d_desc[i] and
 * d_status[i]: the same decisions, the same payload bytes; the fields equal
 * the descriptor form's. */
int cfws_deserialize_slots_info(const void* d_wire, uint64_t wire_size,
                                const uint64_t* d_frame_index, size_t n_frames,
                                uint64_t max_payload, uint64_t slot_bytes,
                                cfws_frame_info_t* d_info, void* d_payload,
                                uint64_t payload_capacity, uint64_t* d_payload_total,
                                void* stream);
int cfws_deserialize_scatter_info(const void* d_wire, uint64_t wire_size,
                                  const uint64_t* d_frame_index, const uint64_t* d_payload_off,
                                  size_t n_frames, uint64_t max_payload, uint64_t max_slot,
                                  cfws_frame_info_t* d_info, void* d_payload,
                                  uint64_t payload_capacity, void* stream);

/* ---- slot receive of a uniform stream ------------------------------------
 * cfws_deserialize_slots_info with the index implicit: frame i is parsed at
 * i * frame_stride, as if d_frame_index[i] = i * frame_stride (the wire
 * cfws_serialize_uniform writes, frame_stride its header + payload bytes).
 * Same decisions, same d_info, payload and total as that indexed call; no
 * index is read. *d_mismatch (may be NULL; the call zeroes it first) = the
 * frames that are not COMPLETE frames of exactly frame_stride wire bytes.
 * Zero means each frame i parsed COMPLETE and ends where frame i + 1 starts:
 * the reference's receive loop (src/ws/co_ws_server.c:107-169 calling
 * co_ws_frame_deserialize, src/ws/co_ws_frame.c:129-247) would have taken
 * the same n frames from the start of the wire. Non-zero: the stream is not
 * uniform there; index it (cfws_index_frames_batch) and use the indexed
 * receive. frame_stride >= 2, n_frames * frame_stride < 2^63. */
int cfws_deserialize_slots_uniform(const void* d_wire, uint64_t wire_size, size_t n_frames,
                                   uint64_t frame_stride, uint64_t max_payload, uint64_t slot_bytes,
                                   cfws_frame_info_t* d_info, void* d_payload,
                                   uint64_t payload_capacity, uint64_t* d_payload_total,
                                   uint32_t* d_mismatch, void* stream);

/* ---- deserialize, each payload to the caller's offset ---------------------
 * cfws_deserialize_slots with payload_off = d_payload_off[i] (the caller's
 * own buffer for each frame, as the reference allocates one per frame,
 * co_ws_frame.c:216-223): one launch, each wire line read once. Every
 * offset must be a multiple of 16; max_slot (a multiple of 16 in [16, 2^31])
 * bounds the payloads. A COMPLETE frame with a non-empty payload gets
 * CFWS_ERROR_OUT_OF_MEMORY when that payload is longer than max_slot, ends
 * past payload_capacity, or has an offset that is not a multiple of 16; its
 * destination is not written. Otherwise as cfws_deserialize_slots: the
 * unmasked payload, then zeros to the next 16-byte boundary (cut at the
 * capacity); nothing else is written. Destinations that overlap are the
 * caller's to avoid. */
int cfws_deserialize_scatter(const void* d_wire, uint64_t wire_size,
                             const uint64_t* d_frame_index, const uint64_t* d_payload_off,
                             size_t n_frames, uint64_t max_payload, uint64_t max_slot,
                             cfws_frame_desc_t* d_desc, int32_t* d_status,
                             void* d_payload, uint64_t payload_capacity, void* stream);

/* ---- split ops: headers and payload XOR as separate passes ---------------
 * The two halves of the codec over frames the caller lays out itself (a send
 * path that gathers headers and payloads into iovecs, a receive path that
 * places payloads in its own buffers): every descriptor names its own source
 * and destination, nothing is packed and no workspace is needed.
 *   cfws_encode_headers: frame i's header (co_ws_frame.c:34-91: b0 = opcode
 *     | fin << 7, minimal 7/16/64-bit length, the 4 key bytes when mask) at
 *     d_wire + wire_off; sets header_size (2..14).
 *   cfws_parse_headers: co_ws_frame_deserialize's header decisions
 *     (co_ws_frame.c:131-213, with the callers' 2-byte precheck,
 *     co_ws_client.c:202-206) at d_frame_index[i] against wire_size: d_desc[i]
 *     (wire_off = the start, payload_off = 0) and d_status[i] -- the decode of
 *     cfws_deserialize_plan without its payload layout.
 *   cfws_mask_batch: the serialize payload loop (co_ws_frame.c:93-97):
 *     d_wire[wire_off + h + k] = d_payload[payload_off + k] ^ key[k % 4],
 *     k < payload_size, h = the header size of (payload_size, mask); a copy
 *     when mask == 0. Header bytes are not touched.
 *   cfws_unmask_batch: the deserialize payload loop (co_ws_frame.c:232-242):
 *     d_payload[payload_off + k] = d_wire[wire_off + header_size + k] ^
 *     key[k % 4] for every frame whose d_status is CFWS_PARSE_COMPLETE
 *     (d_status NULL: every frame); a copy when mask == 0.
 * Destination bytes at or past the capacity are not written. Destination
 * ranges of different frames must not overlap; sources may. max_payload_size
 * is an upper bound of payload_size over the batch: it sizes the grid (a
 * larger frame is still processed, by fewer workgroups). Arenas 16-byte
 * aligned. */
int cfws_encode_headers(cfws_frame_desc_t* d_desc, size_t n_frames, void* d_wire,
                        uint64_t wire_capacity, void* stream);
int cfws_parse_headers(const void* d_wire, uint64_t wire_size, const uint64_t* d_frame_index,
                       size_t n_frames, uint64_t max_payload, cfws_frame_desc_t* d_desc,
                       int32_t* d_status, void* stream);
int cfws_mask_batch(const void* d_payload, const cfws_frame_desc_t* d_desc, size_t n_frames,
                    uint64_t max_payload_size, void* d_wire, uint64_t wire_capacity,
                    void* stream);
/* cfws_mask_batch for frames the caller packed back to back (frame i's
 * header starts where frame i - 1's payload ends, as one co_byte_array of
 * sequential co_ws_frame_serialize calls lays them out) whose headers are
 * the bytes cfws_encode_headers writes. Same result bytes; the 16-byte
 * chunks a frame shares with its neighbour's payload and its own header are
 * then written whole, header bytes included (rewritten with the values
 * cfws_encode_headers wrote), instead of byte by byte after the stream
 * (DESIGN.md §3.8). Each adjacency is checked on the device: a boundary that
 * is not packed, or whose payloads are shorter than 16 bytes, is written as
 * by cfws_mask_batch. */
int cfws_mask_batch_packed(const void* d_payload, const cfws_frame_desc_t* d_desc, size_t n_frames,
                           uint64_t max_payload_size, void* d_wire, uint64_t wire_capacity,
                           void* stream);
int cfws_unmask_batch(const void* d_wire, const cfws_frame_desc_t* d_desc, const int32_t* d_status,
                      size_t n_frames, uint64_t max_payload_size, void* d_payload,
                      uint64_t payload_capacity, void* stream);

/* ---- relay: received frames sent on in one payload pass -------------------
 * What a server does with a frame after co_ws_frame_deserialize: the echo
 * server sends every TEXT / BINARY / CONTINUATION frame back with
 * co_ws_send(ws_client, fin, opcode, data, size) (examples/ws_server/main.c
 * :54-71) and hands every other opcode to co_ws_default_handler
 * (co_ws_client.c:563-600), which answers a PING with co_ws_send_pong on the
 * same payload (:586-591, :552-560). co_ws_send (co_ws_client.c:428-460) is
 * co_ws_frame_serialize with mask = !is_server. cfws_deserialize_batch +
 * cfws_serialize_batch do that in two payload passes through a payload arena;
 * cfws_relay_batch does it in one: out[k] = in[k] ^ key_in[k % 4] ^
 * key_out[k % 4], read from the incoming wire.
 *
 * For i = 0..n_frames-1 in order: co_ws_frame_deserialize's header decisions
 * at d_frame_index[i] against wire_in_size, exactly as cfws_parse_headers
 * takes them (co_ws_frame.c:131-213, with the callers' 2-byte precheck,
 * co_ws_client.c:202-206). If the frame is COMPLETE and `policy` emits it,
 * co_ws_frame_serialize(fin', opcode', out_mask, payload) (co_ws_frame.c
 * :34-97) with key d_out_keys[i] is appended to one byte array: d_wire_out.
 *   CFWS_RELAY_VERBATIM     every COMPLETE frame, with its own fin and opcode.
 *   CFWS_RELAY_ECHO_SERVER  opcodes 0, 1, 2 with their own fin and opcode
 *     (examples/ws_server/main.c:56-62); opcode 9 as fin = 1, opcode 0xA, same
 *     payload (co_ws_client.c:586-591, :552-560); every other opcode emits
 *     nothing -- CLOSE and PONG stay the host's job, which finds them in
 *     d_desc / d_status.
 *   Any other policy: CFWS_ERROR_INVALID_ARGUMENT.
 * d_out_keys is indexed by the input frame i and holds keys in wire order, as
 * cfws_frame_desc_t.mask_key; it may be NULL when out_mask == 0.
 * d_desc[i] / d_status[i] are what cfws_parse_headers writes (wire_off = the
 * start, the incoming key, fin, opcode, mask, header_size, payload_size),
 * except payload_off: the offset in d_wire_out where frame i's outgoing frame
 * starts, i.e. the exclusive prefix sum of the outgoing bytes of frames
 * 0..i-1, written for frames that emit nothing too. There is no capacity
 * status. Bytes at or past out_capacity are not written (nor any byte past
 * the total); *d_out_total (optional) is the unclamped total, as
 * cfws_serialize_* reports it.
 * Indices may repeat and come in any order (a repeated index is the fan-out
 * of one frame). d_wire_in is readable up to round16(wire_in_size); arenas
 * are 16-byte aligned; input and output ranges that overlap are
 * CFWS_ERROR_INVALID_ARGUMENT. Frame-count and size limits are those of
 * cfws_deserialize_plan / cfws_serialize_plan. Nothing is allocated, nothing
 * synchronises. The workspace is cfws_workspace_size(n_frames, out_capacity)
 * plus a 32-byte internal descriptor per frame
 * (cfws_relay_workspace_size: a pure host function). */
#define CFWS_RELAY_VERBATIM     0u
#define CFWS_RELAY_ECHO_SERVER  1u

size_t cfws_relay_workspace_size(size_t n_frames, uint64_t out_capacity);

int cfws_relay_batch(const void* d_wire_in, uint64_t wire_in_size,
                     const uint64_t* d_frame_index, size_t n_frames, uint64_t max_payload,
                     uint32_t policy, uint8_t out_mask, const uint32_t* d_out_keys,
                     cfws_frame_desc_t* d_desc, int32_t* d_status,
                     void* d_wire_out, uint64_t out_capacity, uint64_t* d_out_total,
                     void* d_workspace, size_t workspace_size, void* stream);

/* ---- receive-buffer frame indexing --------
 * The frame walk of the receive loops co_ws_server_on_tcp_receive_ready
 * (co_ws_server.c:107-169) / co_ws_client_on_tcp_receive_ready
 * (co_ws_client.c:200-270) over one connection's received bytes
 * buf[begin, end): from the receive index `begin`, while bytes remain, stop
 * when fewer than 2 are left or a frame does not parse COMPLETE against
 * data_size = end (co_ws_frame_deserialize's decisions, co_ws_frame.c
 * :131-213, with max_payload as co_ws_config_get_max_receive_payload_size).
 * Per connection it reports the starts of the COMPLETE frames, the receive
 * index after them (*consumed, where the reference leaves
 * receive_data.index) and why the walk stopped (*stop):
 *   CFWS_PARSE_COMPLETE      every byte consumed (the loop clears the buffer)
 *   CFWS_PARSE_MORE_DATA     under 2 bytes left, or a frame incomplete: wait
 *   CFWS_ERROR_INVALID_FRAME the frame at *consumed is not WS (HTTP fallback
 *                            / close 1002, co_ws_client.c:62-71)
 *   CFWS_ERROR_DATA_TOO_BIG  the frame at *consumed exceeds max_payload
 *                            (close 1009)
 *   CFWS_INDEX_FULL          host form only: `starts` is full and another
 *                            COMPLETE frame follows; resume at *consumed.
 * The starts feed cfws_deserialize_* (every frame they name is COMPLETE).
 *
 * Host form: one connection, on the calling thread (receive buffers in host
 * memory). Returns the number of starts written. */
#define CFWS_INDEX_FULL 2
size_t cfws_index_frames(const void* h_buf, uint64_t begin, uint64_t end, uint64_t max_payload,
                         uint64_t* starts, size_t max_starts, uint64_t* consumed, int32_t* stop);

/* Device form: n_conns connections of one device arena at once, connection
 * c = d_buf[d_begin[c], d_end[c]). d_first[c] = index of c's first start in
 * d_starts (exclusive prefix sum of the per-connection counts), *d_total =
 * all starts (unclamped); starts at positions >= starts_capacity are not
 * written. d_consumed / d_stop per connection as above. The workspace
 * (cfws_index_workspace_size) holds 64 starts per connection between the
 * walk and the scan that places them: 520 bytes per connection. */
size_t cfws_index_workspace_size(size_t n_conns);
int cfws_index_frames_batch(const void* d_buf, const uint64_t* d_begin, const uint64_t* d_end,
                            size_t n_conns, uint64_t max_payload, uint64_t* d_starts,
                            uint64_t starts_capacity, uint64_t* d_first, uint64_t* d_consumed,
                            int32_t* d_stop, uint64_t* d_total, void* d_workspace,
                            size_t workspace_size, void* stream);

/* ---- handshake accept keys ----------------
 * Sec-WebSocket-Accept for n connections at once, as
 * co_ws_create_base64_accept_key computes it for one
 * (co_ws_http_extension.c:26-57; used by the server's upgrade response :342
 * and the client's check :245): base64(SHA-1(key || "258EAFA5-E914-47DA-
 * 95CA-C5AB0DC85B11")) with '=' padding. Key c is the bytes
 * d_keys[d_key_off[c], d_key_off[c + 1]) (n + 1 offsets, any length); its
 * 28-character accept value + NUL goes to d_accept + CFWS_WS_ACCEPT_SLOT * c
 * (the slot's last 3 bytes are written as zeros when d_accept is 16-byte
 * aligned, and left alone otherwise). Offsets must not decrease: a key with
 * d_key_off[c + 1] < d_key_off[c] gets an all-zero slot (an empty string). */
#define CFWS_WS_ACCEPT_SLOT 32
int cfws_ws_accept_keys_batch(const void* d_keys, const uint64_t* d_key_off, size_t n,
                              char* d_accept, void* stream);

/* ---- the rest of the upgrade's key handling (co_ws_http_extension.c) -------
 * The three calls below allocate nothing, copy nothing from host memory and
 * do not synchronise: their work is queued on `stream`. None is a timed
 * pass: a pending cfws_time_next_pass pair is dropped. CFWS_OK, or
 * CFWS_ERROR_NO_DEVICE / _INVALID_ARGUMENT / _HIP (the device is checked
 * first, then the arguments; a refused call writes nothing). n == 0 writes
 * no per-connection output, but still the counters and *d_next_draw when
 * they are given.
 *
 * cfws_ws_client_keys_batch: the Sec-WebSocket-Key values of n_conns
 * sequential co_http_request_create_ws_upgrade calls (:280-290: co_random of
 * 16 bytes, co_base64_encode with padding) made after first_draw calls of
 * random() since srandom(seed). Connection c's nonce byte j is draw
 * first_draw + 16 c + j of the stream cfws_draw_mask_keys_seeded_at draws
 * from; its key, 22 characters and "==", goes to d_ws_keys + CFWS_WS_KEY_SLOT
 * * c as 24 characters, the NUL and 7 zero bytes. d_expect_accept (may be
 * NULL) gets, per connection, the 32 bytes cfws_ws_accept_keys_batch writes
 * for that key into an aligned output: the value the server's answer must
 * carry. *d_next_draw (may be NULL) = first_draw + 16 n_conns: the first_draw
 * of whatever draws next (cfws_draw_mask_keys_device for the frames those
 * connections then send). Both outputs 16-byte aligned, 32 n_conns bytes;
 * first_draw <= 2^62; n_conns < 2^30. One launch, no workspace; the nonces
 * never go to memory. cfws_ws_client_keys_group_conns: the connections one
 * workgroup produces (a constant of the build).
 *
 * cfws_ws_upgrade_keys_batch: the server's side. Keys as for
 * cfws_ws_accept_keys_batch (the strlen bytes of each header field). d_valid[c]
 * = 1 when co_http_request_validate_ws_upgrade accepts the key (:156-170:
 * co_base64_decode returns true and nonce_length == 16), else 0. The rule is
 * co_base64.c:94-167's, not RFC 4648's: '\n', '\r' and '=' are skipped
 * wherever they stand; A-Z a-z 0-9 + / and also ! - : _ and every byte >=
 * 0x80 are data; any other byte (NUL included) fails; and with L the key's
 * length the key is valid when nothing failed and floor(3 L / 4) - skipped ==
 * 16. d_accept (may be NULL) gets what cfws_ws_accept_keys_batch writes, for
 * every key, valid or not (the response builder hashes whatever the field
 * holds, :342). A key whose offsets decrease gets d_valid 0 and an all-zero
 * accept slot. *d_invalid_count (may be NULL; zeroed by the call) = the keys
 * with d_valid 0.
 *
 * cfws_ws_check_accept_batch: the client's check of the answers (:231-254):
 * d_ok[c] = 1 when strcmp(answer c, expected c) == 0. d_expect_accept holds
 * 32-byte slots with NUL-terminated strings, as the two calls above and
 * cfws_ws_accept_keys_batch write them; answer c is the bytes
 * d_resp[d_resp_off[c], d_resp_off[c + 1]) read as a C string (it ends at
 * its first NUL or at its end). Decreasing offsets compare unequal.
 * *d_fail_count (may be NULL; zeroed by the call) = the zeros in d_ok. */
#define CFWS_WS_KEY_SLOT 32
int cfws_ws_client_keys_batch(uint32_t seed, uint64_t first_draw, size_t n_conns,
                              char* d_ws_keys, char* d_expect_accept,
                              uint64_t* d_next_draw, void* stream);
size_t cfws_ws_client_keys_group_conns(void);
int cfws_ws_upgrade_keys_batch(const void* d_keys, const uint64_t* d_key_off, size_t n,
                               uint8_t* d_valid, char* d_accept,
                               uint32_t* d_invalid_count, void* stream);
int cfws_ws_check_accept_batch(const char* d_expect_accept, const void* d_resp,
                               const uint64_t* d_resp_off, size_t n,
                               uint8_t* d_ok, uint32_t* d_fail_count, void* stream);

/* ---- WebSocket over HTTP/2 (src/ws_http2) ---------------------------------
 * Send: every WS frame of the batch is serialized (cfws_serialize_batch, into
 * d_wire) and carried in HTTP/2 DATA frames of at most max_frame_size payload
 * bytes (0 = the default 16384, co_http2.h:55), END_STREAM on the last DATA
 * frame of each WS frame -- co_http2_stream_send_ws_frame
 * (co_ws_http2_extension.c:166-199) -> co_http2_stream_send_data
 * (co_http2_stream.c:933-1013), DATA layout co_http2_frame.c:33-72 (9-byte
 * header: 24-bit BE length, type 0, flags, 31-bit BE stream id). The flow
 * control window is assumed to admit every frame. *d_h2_total is unclamped.
 * Receive: the DATA frames starting at d_h2_index[i] (one stream, in order)
 * are parsed (co_http2_frame.c:211-300; status per DATA frame below), their
 * payloads pooled into d_pool until END_STREAM (co_http2_stream.c:550-608),
 * and every pooled message goes through co_ws_frame_deserialize against its
 * own size (co_ws_http2_extension.c:134-164): d_msg_desc / d_msg_status get
 * one entry per message (room for n_h2 entries; entries n_messages..n_h2-1
 * are empty: status CFWS_PARSE_MORE_DATA, no payload, no header, payload_off
 * unspecified), payloads land in d_payload as cfws_deserialize_batch lays
 * them out (flags = 0). *n_messages is final on return: the host waits on an
 * event after the device plan, through 64 bytes of mapped pinned memory and
 * an event made once per device of `stream` (where the kernels run; not
 * necessarily the current device). A calling thread borrows them for its
 * lifetime and hands them back at exit, so threads that come and go reuse
 * them. The payload pass may still be running on the stream, as with the
 * other batch calls. When every DATA payload fits pool_capacity the pool is
 * virtual: WS headers are gathered and payload slices copied + unmasked
 * straight out of the DATA frames in one pass, and d_pool is not written;
 * otherwise the pool is materialised first (the capacity rule needs it) and
 * the one-pass form, already queued, stores nothing. */
#define CFWS_H2_DEFAULT_MAX_FRAME_SIZE 16384u
#define CFWS_H2_PARSE_COMPLETE    0     /* co_http.h:40-42 */
#define CFWS_H2_PARSE_MORE_DATA   1
#define CFWS_H2_PARSE_ERROR      (-1)
#define CFWS_H2_NOT_DATA          3     /* a complete non-DATA frame: no bytes */

size_t cfws_h2_serialize_workspace_size(size_t n_frames, uint64_t wire_capacity,
                                        uint64_t h2_capacity, uint32_t max_frame_size);
int cfws_h2_serialize_batch(const void* d_payload, cfws_frame_desc_t* d_desc, size_t n_frames,
                            uint32_t stream_id, uint32_t max_frame_size, void* d_wire,
                            uint64_t wire_capacity, void* d_h2, uint64_t h2_capacity,
                            uint64_t* d_h2_total, void* d_workspace, size_t workspace_size,
                            void* stream);
size_t cfws_h2_deserialize_workspace_size(size_t n_h2_frames, uint64_t pool_capacity,
                                          uint64_t payload_capacity);
int cfws_h2_deserialize_batch(const void* d_h2, uint64_t h2_size, const uint64_t* d_h2_index,
                              size_t n_h2_frames, uint32_t max_frame_size, int32_t* d_h2_status,
                              void* d_pool, uint64_t pool_capacity, uint64_t max_payload,
                              uint32_t align, cfws_frame_desc_t* d_msg_desc,
                              int32_t* d_msg_status, void* d_payload, uint64_t payload_capacity,
                              uint64_t* d_payload_total, size_t* n_messages,
                              void* d_workspace, size_t workspace_size, void* stream);

/* ---- HTTP/2 receive-buffer frame indexing ---------------------------------
 * The frame walk of the reference's HTTP/2 receive loop,
 * co_http2_client_on_tcp_receive_ready (co_http2_client.c:462-541; the
 * server's loop is co_http2_server.c:139ff), over one connection's received
 * bytes buf[begin, end): from the receive index `begin`, while bytes remain,
 * one co_http2_frame_deserialize (co_http2_frame.c:211-533) per step. A real
 * receive buffer carries SETTINGS, WINDOW_UPDATE, PING and HEADERS frames and
 * the frames of other streams (RFC 8441: one WebSocket per stream) between
 * one stream's DATA frames, and usually ends inside a frame. Each step
 * decides, in the reference's order:
 *   1. fewer than 9 bytes left             -> MORE_DATA
 *   2. length > max_frame_size             -> ERROR (:244-247; before 3)
 *   3. fewer than 9 + length bytes left    -> MORE_DATA (:249-253)
 *   4. type > 9                            -> ERROR (:524-527)
 *   5. need > length                       -> ERROR, where need is the payload
 *      bytes the type's fixed fields take: DATA PADDED ? 1 + pad : 0; HEADERS
 *      that + (PRIORITY ? 5 : 0); PRIORITY 5; RST_STREAM 4; SETTINGS 0;
 *      PUSH_PROMISE (PADDED ? 1 + pad : 0) + 4; PING 8; GOAWAY 8;
 *      WINDOW_UPDATE 4; CONTINUATION 0. pad is the byte after the header,
 *      read only when PADDED is set and length >= 1 (PADDED with length 0 ->
 *      ERROR). The reference's behaviour is UNDEFINED for these frames (it
 *      underflows an unsigned length, :281 :316 :331 :445 :483, or reads past
 *      the frame and trips co_assert, co_http2_client.c:471): ERROR is this
 *      library's rule, as for padded DATA in cfws_h2_deserialize_batch.
 *   6. COMPLETE; the receive index moves by what the parse consumed (:530),
 *      not by 9 + length: DATA, HEADERS, PUSH_PROMISE, GOAWAY, CONTINUATION
 *      9 + length; PRIORITY 14; RST_STREAM, WINDOW_UPDATE 13; PING 17;
 *      SETTINGS 9 + 6 * ((length / 6) mod 65536) (the parameter count is a
 *      uint16_t, :391-392). A control frame whose length differs from its
 *      fixed size therefore leaves the next parse inside it, as in the
 *      reference.
 * The stream id is the header's 4 bytes as the reference reads them: the
 * reserved bit is kept (:263-265; co_http2_get_stream looks that value up).
 * max_frame_size 0 = 16384. A frame is selected when (select ==
 * CFWS_H2_INDEX_ALL or its type is 0) and (stream_id == 0 or its stream id as
 * read == stream_id). The walk passes over every COMPLETE frame; only
 * selected frames are reported: starts[k], and info[k] when info is not
 * NULL. *consumed is where the reference leaves receive_data.index; *stop:
 *   CFWS_H2_PARSE_COMPLETE   every byte consumed (also begin >= end: no
 *                            frames, consumed = begin)
 *   CFWS_H2_PARSE_MORE_DATA  the frame at *consumed is incomplete: wait
 *   CFWS_H2_PARSE_ERROR      the frame at *consumed; the reference closes
 *                            the connection with FRAME_SIZE_ERROR
 *                            (co_http2_client.c:526-536)
 *   CFWS_INDEX_FULL          host form only: `starts` is full and another
 *                            SELECTED frame follows, at *consumed (unselected
 *                            frames before it are consumed); resuming from
 *                            *consumed continues the same walk.
 * No byte outside [begin, end) is read. The server's 24-byte connection
 * preface (co_http2_server.c:32-50) is the caller's to skip through `begin`.
 * select above 1: the host form returns 0 starts, stop CFWS_H2_PARSE_ERROR
 * and consumed = begin; the device form CFWS_ERROR_INVALID_ARGUMENT.
 *
 * Host form: one connection, on the calling thread. Returns the number of
 * starts written. */
#define CFWS_H2_INDEX_ALL   0u   /* every COMPLETE frame */
#define CFWS_H2_INDEX_DATA  1u   /* type 0 only */

typedef struct cfws_h2_frame_info {   /* 16 bytes */
    uint32_t stream_id;   /* the 4 bytes as the reference reads them: reserved bit kept */
    uint32_t length;      /* the header's 24-bit length */
    uint32_t advance;     /* what the receive index moves by (rule 6) */
    uint8_t  type, flags;
    uint16_t zero;
} cfws_h2_frame_info_t;

size_t cfws_h2_index_frames(const void* h_buf, uint64_t begin, uint64_t end,
                            uint32_t max_frame_size, uint32_t select, uint32_t stream_id,
                            uint64_t* starts, cfws_h2_frame_info_t* info, size_t max_starts,
                            uint64_t* consumed, int32_t* stop);

/* Device form: n_conns connections of one device arena at once, connection
 * c = d_buf[d_begin[c], d_end[c]), as cfws_index_frames_batch: d_first[c] =
 * index of c's first selected start in d_starts (exclusive prefix sum of the
 * per-connection selected counts), *d_total = all selected frames
 * (unclamped); positions >= starts_capacity are not written, in d_starts and
 * d_info alike. d_info may be NULL; otherwise it must be 16-byte aligned
 * (each record is one 16-byte store). d_consumed / d_stop per connection as
 * above. Nothing is allocated and nothing synchronises; not a timed pass (a
 * pending cfws_time_next_pass pair is dropped). Errors, device check first:
 * null pointers (as cfws_index_frames_batch), select > 1 or a misaligned
 * d_info -> CFWS_ERROR_INVALID_ARGUMENT; workspace too small ->
 * CFWS_ERROR_WORKSPACE; nothing is written. n_conns == 0 writes *d_total = 0
 * only. The workspace (cfws_h2_index_workspace_size) is the WS indexer's: 64
 * starts per connection between the walk and the scan that places them, 520
 * bytes per connection; the records of those 64 are re-derived from the 9
 * header bytes at each kept start, so they cost no workspace.
 * What the output feeds: with select = CFWS_H2_INDEX_DATA and a stream id,
 * d_starts is exactly the "one stream, in order" index
 * cfws_h2_deserialize_batch takes (the other frames still lie in the buffer
 * between the indexed ones, which that call allows). That receive pools
 * until END_STREAM across its whole index, so the starts of several
 * connections go into one call only when each connection's selected frames
 * end with END_STREAM (the last d_info.flags of each connection shows
 * whether they do); otherwise make one call per connection, using d_first.
 * Speed (profiles/h2index/h2_index_bench.jsonl): a
 * tick of 16,384 connections x 64 KiB indexes in about 0.11 ms at 62 DATA
 * frames of 1,041 bytes per connection (9.6 G frames/s; 0.08 ms with d_info
 * NULL, the WS indexer's time for the same frames) and 0.03 ms at 3 frames
 * of 16,393 bytes; cfws_h2_index_frames over the same bytes in host memory
 * on 16 threads took 2.1-2.2 and 0.5-0.6 ms, so the device form is the faster
 * one at both shapes when the buffers are already in device memory. */
size_t cfws_h2_index_workspace_size(size_t n_conns);
int cfws_h2_index_frames_batch(const void* d_buf, const uint64_t* d_begin, const uint64_t* d_end,
                               size_t n_conns, uint32_t max_frame_size, uint32_t select,
                               uint32_t stream_id, uint64_t* d_starts,
                               cfws_h2_frame_info_t* d_info, uint64_t starts_capacity,
                               uint64_t* d_first, uint64_t* d_consumed, int32_t* d_stop,
                               uint64_t* d_total, void* d_workspace, size_t workspace_size,
                               void* stream);

/* ---- HTTP/2 DATA frames of many streams, by message -------------------------
 * The step between cfws_h2_index_frames_batch and cfws_h2_deserialize_batch
 * when a connection carries several streams (RFC 8441: one WebSocket per
 * stream, so their DATA frames interleave): from the indexed records of all
 * streams of all connections, one receive index in which every message's DATA
 * frames are contiguous and end with END_STREAM, which the receive handles as
 * it is. The calls read the records only, never the receive buffer.
 *
 * Input: n_frames records, starts[k] and info[k], as cfws_h2_index_frames /
 * _batch write them with select ALL or DATA and stream_id 0. Connections as
 * for cfws_messages_batch: connection c is records [conn_first[c], c + 1 <
 * n_conns ? conn_first[c + 1] : n_frames) -- the indexer's d_first --
 * non-decreasing, conn_first[0] == 0, a value above n_frames is read as
 * n_frames, empty connections allowed, nothing outside the arrays is read
 * whatever they hold; conn_first == NULL: one connection of all records
 * (n_conns ignored, conn_first_msg may be NULL and is otherwise one entry).
 *
 * The rule (cfws_rules.h: h2_stream_pooled, h2_stream_starts,
 * h2_stream_msg_flags). co_http2_client_on_tcp_receive_ready
 * (co_http2_client.c:462-541) looks the stream up by the id as read
 * (:475-476: the reserved bit is kept, 0x80000001 and 1 are different
 * streams), sends stream 0 to the system handler (:492-495: never pooled) and
 * hands every other DATA frame to that stream's pool, in arrival order, until
 * a frame with END_STREAM delivers the pooled bytes (co_http2_stream.c:550-608).
 *   * A record with type != 0 or stream_id == 0 is ignored: listed nowhere,
 *     changes nothing.
 *   * A connection's other records are grouped by stream_id, arrival order
 *     kept inside each stream. In one stream's sequence every frame with
 *     END_STREAM (flags & 1) closes a message: the frames since the previous
 *     close, or since the stream's first frame in this call (an END_STREAM
 *     frame of length 0 alone is a message of one frame). The frames after the
 *     stream's last END_STREAM are its tail: pooled, not delivered.
 * The ORDER is this library's: closed messages by connection, then stream_id
 * ascending as an unsigned 32-bit value, then arrival; tails by connection,
 * then stream_id. (The reference delivers a connection's messages in the
 * order of their END_STREAM frames: sort by end_frame for that.) Stream state
 * is not modelled (unknown or closed streams, which the reference drops,
 * :478-484; flow-control resets, co_http2_stream.c:497-507): the records name
 * connection and stream, so the caller drops what it does not know. A stream
 * whose pool was open at the end of the previous call continues in this one
 * when the caller carried its tail; the tables describe this
 * call's frames only.
 *
 * Outputs; no capacities: order, order_frame and msgs have room for n_frames
 * entries, and nothing past the counts is written.
 *   counts[0] closed messages M      counts[1] their frames F
 *   counts[2] tails T                counts[3] the tails' frames
 *   counts[4] streams with at least one closed message
 *   msgs[0, M) the closed messages, msgs[M, M + T) the tails.
 *   order[0, F): the starts[] values of the closed messages' frames, copied
 *     as 64-bit values, message after message: with n = F a valid d_h2_index
 *     of cfws_h2_deserialize_batch over the same arena, whose message row m
 *     is msgs[m] and whose *n_messages is M. order[F, F + counts[3]): the
 *     tails' frames the same way (a tail's `first` is a position in order too).
 *   order_frame (may be NULL): the same positions as record indices.
 *   conn_first_msg[c] (may be NULL without conn_first): index of c's first
 *     closed message, the exclusive prefix sum of the per-connection counts.
 *   stream_first[s] (may be NULL; room for n_frames entries): index of the
 *     first closed message of the s-th stream that has one, in table order:
 *     what cfws_messages_batch takes as d_conn_first over the receive's
 *     d_msg_desc, so that WS fragments arriving as separate
 *     END_STREAM-delimited messages of one stream are joined per stream.
 * Host form: on the calling thread (it allocates its sort's scratch); returns
 * M. */
#define CFWS_H2_STREAM_CLOSED  1u   /* ends with END_STREAM: a message            */
#define CFWS_H2_STREAM_TAIL    2u   /* the stream's frames after its last close   */
#define CFWS_H2_STREAM_FIRST   4u   /* first closed message of its (conn, stream) */
#define CFWS_H2_STREAM_PADDED  8u   /* some frame has PADDED: length_sum is an
                                       upper bound of the pooled bytes, else exact */
typedef struct cfws_h2_stream_msg {   /* 32 bytes, two 16-byte stores */
    uint64_t length_sum;   /* sum of the frames' info.length */
    uint32_t first;        /* position of its first frame in d_order */
    uint32_t n_data;       /* its DATA frames */
    uint32_t conn;         /* 0 without conn_first */
    uint32_t stream_id;    /* as read */
    uint32_t end_frame;    /* record index (into starts/info) of its last frame */
    uint8_t  flags, zero8; uint16_t zero16;
} cfws_h2_stream_msg_t;

size_t cfws_h2_streams_from_frames(const uint64_t* starts, const cfws_h2_frame_info_t* info,
        size_t n_frames, const uint64_t* conn_first, size_t n_conns,
        uint64_t* order, uint32_t* order_frame, cfws_h2_stream_msg_t* msgs,
        uint64_t* conn_first_msg, uint64_t* stream_first, uint64_t counts[5]);

/* Device form: the same tables from device-resident records, so that an
 * HTTP/2 tick is index -> group -> one receive -> message tables:
 * cfws_h2_index_frames_batch -> cfws_h2_streams_batch (d_first as
 * d_conn_first) -> read the counts -> one cfws_h2_deserialize_batch over
 * d_order[0, F) -> cfws_messages_batch with d_stream_first. d_msgs must be
 * 16-byte aligned. Nothing is allocated and nothing synchronises; not a timed
 * pass (a pending cfws_time_next_pass pair is dropped); every launch is a
 * plain kernel on `stream` (no look-back between workgroups; their number
 * depends on n_frames alone), so the call can be captured. The result does
 * not depend on what the workspace or the outputs held. Errors, device check
 * first: null d_starts, d_info, d_order or d_msgs (n_frames > 0), d_counts or
 * workspace, d_conn_first_msg (with d_conn_first), a misaligned d_msgs,
 * n_frames > 2^32 - 1 -> CFWS_ERROR_INVALID_ARGUMENT; workspace too small ->
 * CFWS_ERROR_WORKSPACE; nothing is written. n_frames == 0 writes five zero
 * counts and d_conn_first_msg[c] = 0 for every c.
 * The grouping is a stable sort of each connection's DATA records by
 * (stream_id, arrival). The DATA records are compacted into a dense list
 * (connections stay contiguous); every aligned block of
 * cfws_h2_streams_group_frames() dense rows is sorted in LDS by (connection,
 * stream_id, arrival), a bitonic network, which finishes every connection
 * that lies inside one block -- small connections share a workgroup. A
 * connection that crosses a block boundary, as every connection of more than
 * cfws_h2_streams_group_frames() DATA records does, is finished in the
 * workspace: merge passes over its block pieces (run lengths G, 2G, 4G, ...;
 * each key finds its place by a binary search in the sibling run), so a
 * connection of n records costs about n log2(G)^2 / 4 compare-exchanges and
 * at most log2(n / G) + 2 passes of n log2(n) key comparisons whatever the
 * peer interleaves: no path is quadratic, and none ranks by counting. The workspace (cfws_h2_streams_workspace_size) is 76 bytes per
 * record (a 16-byte dense row, three 8-byte key arrays, a 4-byte message
 * index and a 32-byte row per message) and 4 bytes per connection.
 * Speed (profiles/h2streams/h2_streams_bench.jsonl):
 * 16,384 connections x 62 records over 4 streams take 0.27 ms, 16,384 x 3
 * records on one stream 0.15 ms (its 18 launches) and one connection of 2^20
 * records, each its own stream, 0.38 ms: 13 to 32 times what cfws_device_copy
 * takes for the bytes the call must move (24 per record in, 12 per frame and
 * 32 per message out), and 10, 3.5 and 120 times faster than copying the
 * records to pinned memory and running cfws_h2_streams_from_frames on 16
 * threads (2.7, 0.5 and 46 ms). The device form lost at no shape. */
size_t cfws_h2_streams_workspace_size(size_t n_frames, size_t n_conns);
size_t cfws_h2_streams_group_frames(void);
int cfws_h2_streams_batch(const uint64_t* d_starts, const cfws_h2_frame_info_t* d_info,
        size_t n_frames, const uint64_t* d_conn_first, size_t n_conns,
        uint64_t* d_order, uint32_t* d_order_frame, cfws_h2_stream_msg_t* d_msgs,
        uint64_t* d_conn_first_msg, uint64_t* d_stream_first, uint64_t* d_counts,
        void* d_workspace, size_t workspace_size, void* stream);

/* ---- message and control tables of received frames --------------------------
 * What an application consumes after a receive: where each message starts,
 * how long it is, what it is and whether it is whole, and which frames are
 * control frames. The calls read descriptors and statuses only, so they take
 * the outputs of cfws_deserialize_batch / _plan (with
 * CFWS_DESERIALIZE_REASSEMBLE a message is then the bytes [payload_off,
 * payload_off + payload_size) of the payload arena; with flags = 0 the
 * fragments lie where their descriptors say), of cfws_parse_headers, of
 * cfws_relay_batch and cfws_h2_deserialize_batch's d_msg_desc alike.
 *
 * The rule is THIS LIBRARY'S: the reference hands each frame to the
 * application (examples/ws_client/main.c:50-72) and checks no fragment order.
 * A connection's frames are taken in index order; the only state is `open`
 * (a message is unfinished), false at the connection's start.
 *   * A frame whose status is neither CFWS_PARSE_COMPLETE nor
 *     CFWS_ERROR_OUT_OF_MEMORY is ignored: it changes nothing and is listed
 *     nowhere.
 *   * opcode >= 8 is a control frame: its index is appended to the control
 *     list; `open` is untouched (control frames may sit between a message's
 *     fragments, RFC 6455 5.4).
 *   * opcode < 8 is a data frame. With opcode != 0 or !open it starts a
 *     message (an open one ends CFWS_MESSAGE_CUT) that takes this frame's
 *     index, payload_off, opcode and connection; opcode 0 there sets
 *     CFWS_MESSAGE_HEADLESS (the start lies in an earlier call, or the peer
 *     broke the protocol: the caller knows whether that connection's last
 *     call ended OPEN). Otherwise it joins the open message. Either way
 *     payload_size += the frame's, n_fragments++, an OUT_OF_MEMORY frame sets
 *     CFWS_MESSAGE_LOST_BYTES, and open = !fin; fin sets CFWS_MESSAGE_FINAL.
 *   * At the connection's end an open message gets CFWS_MESSAGE_OPEN.
 * Every message carries exactly one of FINAL, CUT and OPEN.
 *
 * Connections: connection c is frames [conn_first[c], c + 1 < n_conns ?
 * conn_first[c + 1] : n_frames) -- cfws_index_frames_batch's d_first, passed
 * straight through when no start was dropped for capacity. Precondition:
 * non-decreasing, conn_first[0] == 0. A value above n_frames is read as
 * n_frames; nothing outside the arrays is read whatever they hold. Empty
 * connections are allowed. conn_first == NULL: one connection of all frames
 * (n_conns is ignored, conn_first_msg may be NULL and is otherwise one entry).
 * Outputs: messages in frame order; conn_first_msg[c] = index of c's first
 * message (the exclusive prefix sum of the per-connection counts; c's open
 * tail, if any, is its last message); the control list in frame order. status
 * NULL: every frame COMPLETE. Totals are unclamped; positions at or past a
 * capacity are not written. control / n_control may be NULL with
 * control_capacity 0. n_frames <= 2^32 - 1.
 *
 * Host form: on the calling thread; returns the number of messages. */
#define CFWS_MESSAGE_FINAL      1u
#define CFWS_MESSAGE_CUT        2u
#define CFWS_MESSAGE_OPEN       4u
#define CFWS_MESSAGE_HEADLESS   8u
#define CFWS_MESSAGE_LOST_BYTES 16u

typedef struct cfws_message {      /* 32 bytes */
    uint64_t payload_off;    /* the first fragment's payload_off */
    uint64_t payload_size;   /* sum of the fragments' payload_size */
    uint32_t first_frame;    /* index of the first fragment in d_desc */
    uint32_t n_fragments;    /* data frames of the message */
    uint32_t conn;           /* 0 without d_conn_first */
    uint8_t  opcode, flags;
    uint16_t zero;
} cfws_message_t;

size_t cfws_messages_from_frames(const cfws_frame_desc_t* h_desc, const int32_t* h_status,
                                 size_t n_frames, const uint64_t* h_conn_first, size_t n_conns,
                                 cfws_message_t* msgs, size_t msg_capacity,
                                 uint64_t* conn_first_msg, uint32_t* control,
                                 size_t control_capacity, uint64_t* n_control);

/* Device form: the same tables from device-resident descriptors, so that one
 * tick of a many-connection server stays on the device:
 * cfws_index_frames_batch -> cfws_deserialize_batch(REASSEMBLE) ->
 * cfws_messages_batch (d_first as d_conn_first) -> the application's kernel
 * over whole messages; the host reads back *d_n_messages and the short
 * control list. d_msgs must be 16-byte aligned (a record is two 16-byte
 * stores). Nothing is allocated and nothing synchronises; not a timed pass (a
 * pending cfws_time_next_pass pair is dropped); every launch is a plain
 * kernel on `stream` (reduce -> scan of the block sums -> apply, twice, then
 * a pass over messages and one over connections: no look-back between
 * workgroups), so the call can be captured. Errors, device check first: null
 * d_desc (n_frames > 0), d_msgs (msg_capacity > 0), d_control
 * (control_capacity > 0), d_conn_first_msg (with d_conn_first), d_n_messages
 * or workspace, a misaligned d_msgs, n_frames > 2^32 - 1 ->
 * CFWS_ERROR_INVALID_ARGUMENT; workspace too small -> CFWS_ERROR_WORKSPACE;
 * nothing is written. n_frames == 0 writes both totals as 0 and
 * d_conn_first_msg[c] = 0 for every c. The result does not depend on what
 * the workspace or the outputs held. The workspace
 * (cfws_messages_workspace_size) is 48 bytes per frame: a 16-byte row per
 * data frame and a 32-byte row per message between the passes.
 * cfws_messages_group_frames: the frames one workgroup takes, for tests that
 * place messages across its boundaries.
 * Speed (profiles/messages/messages_bench.jsonl):
 * 16,777,216 single-frame messages over 16,384 connections take 1.63 ms
 * (10.3 G frames/s), 9.7 times what cfws_device_copy takes for the bytes the
 * call must move (36 per frame in, 32 per message out), and a tenth of what
 * a caller paid before: 10.6 ms to copy d_desc + d_status into pinned memory
 * plus 5.5 ms of cfws_messages_from_frames on 16 threads. Config 3's batch
 * (292,370 frames, 65,109 messages, one connection) takes 40 us against
 * 0.2 + 1.0 ms. The device form lost at neither shape. */
size_t cfws_messages_workspace_size(size_t n_frames, size_t n_conns);
size_t cfws_messages_group_frames(void);
int cfws_messages_batch(const cfws_frame_desc_t* d_desc, const int32_t* d_status, size_t n_frames,
                        const uint64_t* d_conn_first, size_t n_conns, cfws_message_t* d_msgs,
                        uint64_t msg_capacity, uint64_t* d_conn_first_msg, uint64_t* d_n_messages,
                        uint32_t* d_control, uint64_t control_capacity, uint64_t* d_n_control,
                        void* d_workspace, size_t workspace_size, void* stream);

/* ---- UTF-8 check of received text messages --------------------------------
 * What an RFC 6455 endpoint owes every received text message before handing
 * it on (5.6, 8.1: close 1007 when it is not UTF-8), over the rows that
 * cfws_messages_from_frames / cfws_messages_batch write and the payload arena
 * of the receive. The rule is THIS LIBRARY'S: the reference validates no
 * text. Well-formed UTF-8 is Unicode Table 3-7 / RFC 3629: no overlong forms,
 * no surrogates, nothing above U+10FFFF, no leads C0, C1, F5..FF.
 *
 * Precondition: a checked message's bytes are the contiguous range
 * [payload_off, payload_off + payload_size) of the arena (the REASSEMBLE
 * layout, or a single-fragment message in any layout).
 *
 * Message m is checked when its opcode is 1 (TEXT), or its opcode is 0 with
 * CFWS_MESSAGE_HEADLESS and carry_in != NULL and carry_in[m] &
 * CFWS_UTF8_CARRY_TEXT (it continues a text message of an earlier call: only
 * the caller knows that); and CFWS_MESSAGE_LOST_BYTES is not set; and
 * payload_off + payload_size does not overflow and is <= payload_bytes. Any
 * other message gets an all-zero row and none of its bytes are read.
 *
 * For a checked message the string S is the k carried bytes (k = bits 24..25
 * of carry_in[m], byte j in bits 8j..8j+7; HEADLESS messages only, else and
 * without carry_in k = 0) followed by the message's bytes. With `start` the
 * length of S's longest well-formed prefix, S is VALID (start == len),
 * TRUNCATED (S[start:] is 1-3 bytes that begin a well-formed sequence: the
 * string ends inside a character) or INVALID. prefix = max(start, k) - k;
 * carry = S[start:] when TRUNCATED (what the connection's next call takes as
 * carry_in, with CFWS_UTF8_CARRY_TEXT set by the caller), else 0; flags =
 * CHECKED, one of VALID / TRUNCATED / INVALID, and BAD for INVALID or for
 * TRUNCATED in a message that is not CFWS_MESSAGE_OPEN. A checked message of
 * no bytes and no carry is VALID with prefix 0.
 *
 * Outputs: result[m] for every m; bad[]: the indices of the BAD messages,
 * ascending, positions at or past bad_capacity not written (bad may be NULL
 * with capacity 0); counts[0] = checked messages, counts[1] = BAD messages,
 * both unclamped. Rows may repeat or overlap. The host form runs on the
 * calling thread and returns counts[1] (counts may be NULL). */
#define CFWS_UTF8_CHECKED    1u   /* a text message whose bytes were read */
#define CFWS_UTF8_VALID      2u
#define CFWS_UTF8_TRUNCATED  4u
#define CFWS_UTF8_INVALID    8u
#define CFWS_UTF8_BAD       16u   /* INVALID, or TRUNCATED in a message that is
                                     not CFWS_MESSAGE_OPEN: close 1007 */
#define CFWS_UTF8_CARRY_TEXT 0x80000000u

typedef struct cfws_utf8_result {   /* 16 bytes, one 16-byte store */
    uint64_t prefix;   /* bytes of THIS message's range that precede `start` */
    uint32_t carry;    /* TRUNCATED: S[start:], byte j in bits 8j..8j+7, count
                          in bits 24..25; otherwise 0 */
    uint8_t  flags, zero8;
    uint16_t zero16;
} cfws_utf8_result_t;

size_t cfws_utf8_check_messages(const void* h_payload, uint64_t payload_bytes,
                                const cfws_message_t* h_msgs, size_t n_msgs, const uint32_t* h_carry_in,
                                cfws_utf8_result_t* result, uint32_t* bad, size_t bad_capacity,
                                uint64_t counts[2]);

/* Device form: the receive tick's last library step,
 * cfws_index_frames_batch -> cfws_deserialize_batch(REASSEMBLE) ->
 * cfws_messages_batch -> cfws_utf8_messages_batch -> the application's kernel.
 * Nothing is allocated and nothing synchronises; not a timed pass (a pending
 * cfws_time_next_pass pair is dropped); plain kernels on `stream`, no
 * look-back between workgroups, so the call can be captured. A table pass
 * over the messages cuts each checked one into pieces of
 * cfws_utf8_piece_bytes() (16 lanes x a 16-byte chunk, aligned to the arena's
 * chunks) and scans the counts; the check kernel strides over the pieces, a
 * wave taking cfws_utf8_wave_bytes() and a workgroup
 * cfws_utf8_workgroup_bytes() per stride; a second table pass over the
 * messages writes the rows, the BAD list and the counts. Reads: only 16-byte
 * aligned chunks of the arena that hold a byte of a checked message (the
 * arena is readable to round16(payload_bytes)), never a byte before
 * d_payload; whatever the rows hold, nothing outside the arena and the arrays
 * is touched. Errors, device check first: null d_msgs or d_result
 * (n_msgs > 0), d_payload (payload_bytes > 0), d_bad (bad_capacity > 0),
 * d_counts or workspace, d_result or d_payload not 16-byte aligned,
 * n_msgs > 2^32 - 1 -> CFWS_ERROR_INVALID_ARGUMENT; workspace too small ->
 * CFWS_ERROR_WORKSPACE; nothing is written. n_msgs == 0 writes two zero
 * counts. The result does not depend on what the workspace
 * (cfws_utf8_workspace_size: 16 bytes per message) or the outputs held.
 * Speed (profiles/utf8/utf8_bench.jsonl; 4 GiB of
 * text per shape, every message TEXT): 16,777,216 messages of 256 B take
 * 4.56 ms when all ASCII and 9.38 ms with 1- to 4-byte characters (9.39 ms
 * with one message in a hundred bad); config 3's 65,109 messages 2.30 and
 * 6.26 ms; 65,536 of 64 KiB 2.34 and 6.75 ms. cfws_device_copy of the same
 * number of bytes, which reads and writes what this call only reads, takes
 * 1.31 ms: the call is 1.8 to 3.5 copies on ASCII and 4.8 to 7.2 on other
 * text, where the check kernel's arithmetic (every non-ASCII byte judged one
 * after the other per lane) holds it, not memory. What a caller paid before,
 * 75 ms to copy the text into pinned memory plus cfws_utf8_check_messages on
 * 16 threads (18-25 ms ASCII, 0.81-0.83 s other text), is 22 to 143 calls.
 * The device form lost at no shape. */
size_t cfws_utf8_workspace_size(size_t n_msgs);
size_t cfws_utf8_piece_bytes(void);
size_t cfws_utf8_wave_bytes(void);
size_t cfws_utf8_workgroup_bytes(void);
int cfws_utf8_messages_batch(const void* d_payload, uint64_t payload_bytes, const cfws_message_t* d_msgs,
                             size_t n_msgs, const uint32_t* d_carry_in, cfws_utf8_result_t* d_result,
                             uint32_t* d_bad, uint64_t bad_capacity, uint64_t* d_counts,
                             void* d_workspace, size_t workspace_size, void* stream);

/* ---- host-memory pipeline ------------------------------------------------
 * The same codec over HOST buffers (socket send/receive side): the batch is
 * cut into chunks of frames; `depth` slots (1..4), each with a stream and
 * device staging of chunk_bytes per direction, overlap H2D, the device plan +
 * kernels and D2H of consecutive chunks. Host buffers should be pinned.
 * Synchronous: results are in host memory on return. On an error return no
 * copy is in flight either (the caller's buffers may be freed or reused), the
 * outputs' contents are unspecified, and the pipeline may be used again.
 * max_frames bounds the frames per chunk (descriptor staging). */
typedef struct cfws_pipeline cfws_pipeline_t;
int cfws_pipeline_create(uint64_t chunk_bytes, size_t max_frames, int depth,
                         cfws_pipeline_t** out);
void cfws_pipeline_destroy(cfws_pipeline_t* pipeline);
/* cfws_serialize_batch over host arenas; h_desc gets wire_off/header_size. */
int cfws_pipeline_serialize(cfws_pipeline_t* pipeline, const void* h_payload,
                            cfws_frame_desc_t* h_desc, size_t n_frames, void* h_wire,
                            uint64_t wire_capacity, uint64_t* wire_total);
/* cfws_deserialize_batch over host buffers, flags = 0 (the reassembly layout
 * needs the whole batch). Precondition: h_frame_index increasing, every
 * frame ending at or before the next start (what a receive loop's index
 * satisfies). */
int cfws_pipeline_deserialize(cfws_pipeline_t* pipeline, const void* h_wire,
                              uint64_t wire_size, const uint64_t* h_frame_index,
                              size_t n_frames, uint64_t max_payload, uint32_t align,
                              uint32_t flags, cfws_frame_desc_t* h_desc, int32_t* h_status,
                              void* h_payload, uint64_t payload_capacity,
                              uint64_t* payload_total);
/* The receive loop over one host buffer h_wire[begin, end): cfws_index_frames
 * (on the calling thread) then cfws_pipeline_deserialize of the COMPLETE
 * frames it found. *n_frames: in, the capacity of h_desc / h_status; out,
 * the frames deserialized. *consumed / *stop as cfws_index_frames reports
 * them (CFWS_INDEX_FULL: more frames follow; call again from *consumed). */
int cfws_pipeline_receive(cfws_pipeline_t* pipeline, const void* h_wire, uint64_t begin,
                          uint64_t end, uint64_t max_payload, uint32_t align,
                          cfws_frame_desc_t* h_desc, int32_t* h_status, size_t* n_frames,
                          uint64_t* consumed, int32_t* stop, void* h_payload,
                          uint64_t payload_capacity, uint64_t* payload_total);

/* WebSocket over HTTP/2 through host memory: cfws_h2_serialize_batch /
 * cfws_h2_deserialize_batch per chunk, with the copies overlapped as above.
 * Send: h_desc gets header_size / wire_off; *h2_total = DATA-stream bytes
 * (unclamped). Receive: h_h2_status[i] per DATA frame, one message entry per
 * pooled message (room for n entries), *n_messages, payloads laid out as the
 * batch call lays them out; chunks end where no message is open, so a
 * message larger than the chunk is an error. The index precondition of
 * cfws_pipeline_deserialize holds for DATA frames too. */
int cfws_pipeline_h2_serialize(cfws_pipeline_t* pipeline, const void* h_payload,
                               cfws_frame_desc_t* h_desc, size_t n, uint32_t stream_id,
                               uint32_t max_frame_size, void* h_h2, uint64_t h2_capacity,
                               uint64_t* h2_total);
int cfws_pipeline_h2_deserialize(cfws_pipeline_t* pipeline, const void* h_h2, uint64_t h2_size,
                                 const uint64_t* h_index, size_t n, uint32_t max_frame_size,
                                 uint64_t max_payload, uint32_t align, int32_t* h_h2_status,
                                 cfws_frame_desc_t* h_msg_desc, int32_t* h_msg_status,
                                 size_t* n_messages, void* h_payload, uint64_t payload_capacity,
                                 uint64_t* payload_total);
/* The HTTP/2 receive loop over one connection's host buffer h_h2[begin, end)
 * for one stream: cfws_h2_index_frames(select = CFWS_H2_INDEX_DATA,
 * stream_id) on the calling thread, then cfws_pipeline_h2_deserialize of the
 * DATA frames it found with h2_size = *consumed (bytes past the walk's stop
 * are never staged). The plain composition: the walk finishes before the
 * first chunk is staged (it is not interleaved with the chunks as
 * cfws_pipeline_receive's is). *n_frames: in, the capacity of h_h2_status /
 * h_msg_desc / h_msg_status; out, the DATA frames indexed. *consumed / *stop
 * as cfws_h2_index_frames reports them (CFWS_INDEX_FULL: another DATA frame
 * of the stream follows at *consumed; call again from there; each call
 * pools its own DATA frames only, as cfws_pipeline_h2_deserialize does, so
 * size the capacity to end where messages do). */
int cfws_pipeline_h2_receive(cfws_pipeline_t* pipeline, const void* h_h2, uint64_t begin,
                             uint64_t end, uint32_t stream_id, uint32_t max_frame_size,
                             uint64_t max_payload, uint32_t align, int32_t* h_h2_status,
                             cfws_frame_desc_t* h_msg_desc, int32_t* h_msg_status,
                             size_t* n_frames, size_t* n_messages, uint64_t* consumed,
                             int32_t* stop, void* h_payload, uint64_t payload_capacity,
                             uint64_t* payload_total);

/* How the pipeline's D2H leg moves bytes into a MAPPED host output arena
 * (hipHostMalloc(..., hipHostMallocMapped)); unmapped arenas always take
 * SDMA. AUTO (the default): a kernel storing into the arena for serialize,
 * an SDMA copy for deserialize -- each direction's faster choice beside the
 * in-order H2D copies. DMA: SDMA both ways; KERNEL:
 * the kernel both ways. The environment variable CFWS_PIPELINE_D2H = auto |
 * dma | kernel sets the default of new pipelines. */
#define CFWS_PIPELINE_D2H_AUTO   0
#define CFWS_PIPELINE_D2H_DMA    1
#define CFWS_PIPELINE_D2H_KERNEL 2
int cfws_pipeline_set_d2h(cfws_pipeline_t* pipeline, int mode);

/* D2H by a kernel: copies d_src[0, n) to h_dst, a host buffer allocated (or
 * registered) MAPPED (hipHostMalloc(..., hipHostMallocMapped)), by 16-byte
 * stores over PCIe: the pipeline's D2H leg in CFWS_PIPELINE_D2H_KERNEL mode
 * (and serialize's in AUTO). CFWS_ERROR_INVALID_ARGUMENT when h_dst is
 * not mapped memory. cfws_mapped_device_pointer: h_ptr's device address when
 * it is mapped HIP host memory, else NULL. */
int cfws_copy_to_host(const void* d_src, void* h_dst, uint64_t n, void* stream);
void* cfws_mapped_device_pointer(const void* h_ptr);

/* ---- HIP graphs of a batch (cfws_graph.cpp) ------------------------------
 * A batch shape replayed over the same arenas: cfws_serialize_batch /
 * cfws_deserialize_batch with these exact arguments, captured once into a
 * hipGraph and launched with one call on any stream. Pointers, frame count
 * and capacities are fixed at capture; descriptor contents and payload /
 * wire bytes may change between launches (the plans run on the device at
 * every launch). For small batches, where launch latency rather than HBM
 * bounds a call. cfws_h2_deserialize_batch
 * synchronises and cannot be captured. */
typedef struct cfws_graph cfws_graph_t;
int cfws_graph_serialize(const void* d_payload, cfws_frame_desc_t* d_desc, size_t n, void* d_wire,
                         uint64_t wire_capacity, uint64_t* d_wire_total, void* d_workspace,
                         size_t workspace_size, cfws_graph_t** graph);
int cfws_graph_deserialize(const void* d_wire, uint64_t wire_size, const uint64_t* d_index, size_t n,
                           uint64_t max_payload, uint32_t align, uint32_t flags,
                           cfws_frame_desc_t* d_desc, int32_t* d_status, void* d_payload,
                           uint64_t payload_capacity, uint64_t* d_payload_total, void* d_workspace,
                           size_t workspace_size, cfws_graph_t** graph);
int cfws_graph_launch(cfws_graph_t* graph, void* stream);
void cfws_graph_destroy(cfws_graph_t* graph);

/* ---- single-buffer XOR (used by the per-frame drop-in path) --------------
 * d_dst[i] = d_src[i] ^ key byte (i + key_phase) % 4, i < n. */
int cfws_xor_mask(const void* d_src, void* d_dst, uint64_t n, uint32_t mask_key,
                  uint32_t key_phase, void* stream);

/* Mask keys for a batch, drawn exactly as sequential co_ws_frame_serialize
 * calls would draw them: 4 x (random() % 256) per frame whose mask flag is
 * set, in frame order, from the process's current random() state
 * (co_ws_frame.c:84 -> src/core/co_random.c:32-35). mask_flags == NULL
 * means every frame is masked; unmasked frames get key 0. Host memory. */
void cfws_draw_mask_keys(size_t n_frames, const uint8_t* mask_flags, uint32_t* keys);
/* The keys the same calls draw right after srandom(seed), taken from a
 * private copy of that generator (glibc random_r): other threads' rand() /
 * random() calls cannot interleave with the draws, and the process's
 * random() state is not touched. CFWS_OK, or CFWS_ERROR_INVALID_ARGUMENT. */
int cfws_draw_mask_keys_seeded(uint32_t seed, size_t n_frames, const uint8_t* mask_flags,
                               uint32_t* keys);
/* The same stream entered at a position: the keys cfws_draw_mask_keys_seeded
 * (seed, ...) would give frames that come after first_draw calls of random()
 * since srandom(seed). The masked frame of rank m (counting masked frames
 * only) gets byte j = draw first_draw + 4 m + j; unmasked frames get 0 and
 * draw nothing. *next_draw (may be NULL) = first_draw + 4 x masked frames:
 * the first_draw of the batch that follows. first_draw <= 2^62, and need not
 * be a multiple of 4 (other users of random(), such as the handshake key,
 * move the stream by other amounts). The generator is linear, so the call
 * jumps to the position (a few dozen 31 x 31 products) and discards
 * nothing. first_draw = 0 is cfws_draw_mask_keys_seeded. Host memory; the
 * process's random() state is not touched. CFWS_OK, or
 * CFWS_ERROR_INVALID_ARGUMENT (first_draw, or keys NULL with n_frames > 0). */
int cfws_draw_mask_keys_seeded_at(uint32_t seed, uint64_t first_draw, size_t n_frames,
                                  const uint8_t* mask_flags, uint32_t* keys, uint64_t* next_draw);
/* The device form: the same keys into d_keys and the same next position into
 * *d_next_draw (device memory, may be NULL), queued on `stream`. Nothing is
 * allocated, copied from host memory or synchronised. d_mask_flags == NULL:
 * every frame masked, one launch, no workspace. With d_mask_flags (device,
 * readable to round16(n_frames) bytes) the call needs d_workspace of
 * cfws_draw_keys_workspace_size(n_frames) bytes, 16-byte aligned; its
 * contents on entry do not matter. d_keys is 16-byte aligned and exactly
 * 4 x n_frames bytes of it are written. n_frames < 2^32. n_frames = 0
 * writes no key and *d_next_draw = first_draw. Not a timed pass: a pending
 * cfws_time_next_pass pair is dropped. CFWS_OK, or
 * CFWS_ERROR_INVALID_ARGUMENT / _WORKSPACE / _NO_DEVICE / _HIP.
 * cfws_draw_keys_group_frames: the frames one workgroup draws (a constant of
 * the build; the sizes at which the kernel's paths change are its multiples). */
size_t cfws_draw_keys_workspace_size(size_t n_frames);
int cfws_draw_mask_keys_device(uint32_t seed, uint64_t first_draw, size_t n_frames,
                               const uint8_t* d_mask_flags, uint32_t* d_keys, uint64_t* d_next_draw,
                               void* d_workspace, size_t workspace_size, void* stream);
size_t cfws_draw_keys_group_frames(void);

/* Frees the calling thread's drop-in staging buffers and stream
 * (cfws_frame.cpp) now; optional: a thread that exits without calling it
 * hands them back for reuse by later threads. */
void cfws_release_thread_resources(void);

/* Device policy of the drop-in co_ws_frame_* calls (cfws_frame.cpp). By
 * default (device -1) a thread's masked frames run on its current HIP device,
 * read on every frame. cfws_bind_thread_device(d) pins the calling thread to
 * device d whatever its current device is, so a server with one co_thread
 * per GPU (the reference hands accepted sockets to other threads,
 * co_net_worker.c:240) can spread its connections over the GPUs. A thread
 * whose device changes hands its stream and staging buffers back to a
 * per-device pool and borrows the new device's. CFWS_OK, or
 * CFWS_ERROR_INVALID_ARGUMENT / CFWS_ERROR_NO_DEVICE (d not a gfx950).
 * cfws_thread_device returns the device the next frame would use (-1 on
 * error). */
int cfws_bind_thread_device(int device);
int cfws_thread_device(void);

/* Size policy of the drop-in co_ws_frame_* calls (cfws_frame.cpp). A masked
 * payload of fewer than `bytes` bytes is XORed on the calling thread by the
 * library's own vector loop; payloads of `bytes` or more go to the device
 * (the frame service up to 32 KiB, a launch per frame above). Measured per
 * frame on the MI355X box, the calling thread is faster
 * at every size from 125 B to 4 MiB and spends less CPU time: a per-frame
 * device call copies the payload into and out of pinned staging on the
 * calling thread and waits on PCIe, and its wait spins (or, blocked on an
 * event, cost as much thread CPU time). So the default keeps every frame on
 * the calling thread and the device is opt-in: CFWS_DROPIN_GPU_MIN_DEFAULT
 * is SIZE_MAX; the CFWS_DROPIN_GPU_MIN environment variable (read at load)
 * or this call sets another threshold, 0 sends every masked frame to the
 * device. A frame below the threshold makes no HIP call and needs no
 * device; a frame at or above it fails without a gfx950 agent.
 * Process-wide. The batch ABI above has no host path at any size. */
#define CFWS_DROPIN_GPU_MIN_DEFAULT ((size_t)-1)
void cfws_set_dropin_gpu_min(size_t bytes);
size_t cfws_dropin_gpu_min(void);

/* ---- streaming device copy ------------------------------------------------
 * d_dst[i] = d_src[i], i < n: a bare HBM stream (the bench's copy ceiling,
 * the read + write shape of the codec without its frames). Pointers and n
 * multiples of 16. */
int cfws_device_copy(const void* d_src, void* d_dst, uint64_t n, void* stream);

/* ---- profiling ------------------------------------------------------------
 * `start` / `stop` (hipEvent_t) for the CALLING THREAD's next batch call
 * (any function above that takes a stream). That call takes the pair on
 * entry -- from then on no pair is pending -- and records `start` on its
 * stream right before its timed pass and `stop` right after it:
 *   cfws_serialize_batch / _execute, cfws_deserialize_batch / _execute:
 *     the streaming pass (xform_kernel with its edge workgroups; both
 *     passes of a reassembling execute are one timed span); for batches of
 *     small frames the one kernel the call launches instead (the small-batch
 *     kernel, or the fused plan + copy kernel of cfws_deserialize_batch);
 *   cfws_deserialize_slots / _scatter: their one kernel;
 *   cfws_h2_serialize_batch: its DATA-frame pass; cfws_h2_deserialize_batch:
 *     its fused payload pass, or, when the pooled bytes exceed pool_capacity
 *     (that pass then stores nothing), the pool + plan + payload passes of
 *     the general form that does the work.
 * Any other call, an error return, an empty batch, a graph capture / launch
 * or a pipeline call records nothing and drops the pair. NULL, NULL clears
 * a pending pair. Lets a caller time the one kernel of a multi-kernel call
 * that moves the bytes (bench.py's roofline figures). */
int cfws_time_next_pass(void* start, void* stop);

/* The kernel cfws_deserialize_batch's timed pass is for a call with these
 * sizes (its pointers valid): "deserialize_small_kernel" (one launch for a
 * small batch), "deserialize_plan_single_kernel<true>" (the fused plan +
 * copy of batches of small frames) or "xform_kernel<1>" (the execute after
 * the plan). The same rule the call applies, so a profile can name what it
 * timed. A static string. */
const char* cfws_deserialize_pass_kernel(size_t n_frames, uint64_t wire_size, uint32_t align,
                                         uint32_t flags, uint64_t payload_capacity);

/* The kernel the slot / scatter receives (cfws_deserialize_slots*,
 * cfws_deserialize_scatter*) launch for n_frames frames in wire_size bytes
 * and slots (max_slot) of slot_bytes: "deserialize_slots_piece_kernel" (one
 * wave per 2 KiB piece of a frame's slot: slots over 8,160 bytes whose frames
 * average over 1,040 bytes, and from 2 KiB slots that are multiples of 128
 * filling at least 85 % of their pieces, with frames averaging 85 % of the
 * slot), "deserialize_slots_kernel" (short frames in large slots: frames
 * averaging up to 1,040 bytes in slots over 8,160 bytes; frames of up to 1 KiB
 * filling under half their slot, or under 80 % of a slot of 1 KiB or more)
 * or "deserialize_slots_window_kernel" (the rest). The calls' own rule. A
 * static string. */
const char* cfws_deserialize_slots_pass_kernel(size_t n_frames, uint64_t wire_size, uint64_t slot_bytes);

/* The kernel cfws_serialize_uniform launches for frames of payload_size
 * bytes (masked or not): "serialize_uniform_small_kernel" (payloads of
 * 32-65,535 bytes, multiples of 16), "serialize_uniform_kernel" (other
 * frames of at least 32 wire bytes) or "serialize_uniform_bytes_kernel".
 * The call's own rule. A static string. */
const char* cfws_serialize_uniform_pass_kernel(uint64_t payload_size, uint8_t mask);

/* ---- synthetic input (bench / tests) -------------------------------------
 * d_dst[i] = byte ((byte_base + i) % 8) of splitmix64 output number
 * (byte_base + i) / 8 for `seed`; byte_base must be a multiple of 8. */
int cfws_fill_splitmix(void* d_dst, uint64_t n_bytes, uint64_t seed,
                       uint64_t byte_base, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CFWS_H */
