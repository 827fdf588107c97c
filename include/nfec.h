/*
 * nfec.h -- C ABI of the MI355X-native NORM FEC engine (libnfec.so).
 *
 * Drop-in boundary for NORM's FEC plugin layer (reference include/normEncoder.h:38-54):
 * plain pointers, sizes and integer status codes; no C++ or torch types cross it.
 * Every compute entry point runs hand-written gfx950 HIP kernels (a missing/failed GPU yields
 * NFEC_EDEVICE; nothing falls back to the CPU), except the per-call entry points named *_host
 * ("host CPU per-call paths" below), which are the host path by definition: one Encode call of
 * NORM's incremental sender, or one block's repair, is microseconds of work, less than a GPU
 * round trip.  Which of the two a drop-in class calls is its documented policy, not a fallback.
 *
 * Reference interfaces each entry replaces (paths in USNavalResearchLaboratory/norm):
 *   nfec_codec_create(_ex) NormEncoderRS8::Init  src/common/normEncoderRS8.cpp:400-462
 *                         NormDecoderRS8::Init   src/common/normEncoderRS8.cpp:542-649
 *                         NormEncoderRS16::Init  src/common/normEncoderRS16.cpp:399-461
 *                         NormEncoderMDP::Init   src/common/normEncoderMDP.cpp:56-84
 *   nfec_codec_destroy    NormEncoderXX::Destroy / NormDecoderXX::Destroy (e.g. normEncoderRS8.cpp:464-471)
 *   nfec_encode           the per-segment NormEncoder::Encode loop as run by
 *                         NormObject::CalculateBlockParity  src/common/normObject.cpp:2203-2229
 *                         (NormEncoderRS8::Encode normEncoderRS8.cpp:473-483, RS16 :472-482,
 *                          MDP normEncoderMDP.cpp:178-211) for many blocks at once
 *   nfec_decode           NormDecoder::Decode  (RS8 normEncoderRS8.cpp:652-757, RS16 :650-755,
 *                         MDP normEncoderMDP.cpp:333-430) for many blocks at once, as called
 *                         from NormObject::HandleObjectMessage src/common/normObject.cpp:1548-1644
 *   nfec_rx_place / nfec_decode_received
 *                         the segment copy, the reception mask and the erasure list of
 *                         NormObject::HandleObjectMessage  src/common/normObject.cpp:1548-1644
 *   nfec_rx_ingest        the same with the FEC payload ID read from the message where it lies
 *                         (NormPayloadId::GetFecBlockId / GetFecSymbolId / GetFecBlockLength,
 *                         include/normMessage.h:485-544)
 *   nfec_tx_list / nfec_tx_emit
 *                         the pending walk, the payload lengths, the FEC payload ID and UnsetPending
 *                         of NormObject::NextSenderMsg  src/common/normObject.cpp:1877-2078
 *   nfec_tx_emit_data / nfec_rx_ingest_data
 *                         the same two with the whole NORM_DATA message: the header NextSenderMsg and
 *                         NormSession::SendMessage write (normObject.cpp:1808-1857, normSession.cpp:4923-4924,
 *                         :5013) and the validation of NormMsg::InitFromBuffer  src/common/normMessage.cpp:17-92
 *   nfec_tx_handle_nacks / nfec_tx_activate_repairs / nfec_tx_end_blocks
 *                         NormSession::SenderHandleNackMessage (!holdoff)  src/common/normSession.cpp:3706-4300,
 *                         NormBlock::HandleSegmentRequest  src/common/normSegment.cpp:341-402, OnRepairTimeout
 *                         normSession.cpp:4720-4750 and ResetParityCount  src/common/normObject.cpp:2079-2083
 *   nfec_object_layout_for / nfec_object_read / nfec_object_write
 *                         the block partition of NormObject::Open  src/common/normObject.cpp:134-137,
 *                         :203-231, NormDataObject::ReadSegment :2673-2718 and WriteSegment :2628-2670
 *   nfec_stream_frame / nfec_stream_pack / nfec_stream_unpack
 *                         NormStreamObject::Write  src/common/normObject.cpp:4039-4232, the stream
 *                         payload header include/normMessage.h:1145-1196, ReadPrivate :3700-3860
 *   nfec_encode_host_vectors / nfec_decode_host_vectors
 *                         the same two sites on NORM's scattered segment lists (block->SegmentList())
 *   nfec_encode_segment   NormEncoder::Encode(segmentId, dataVector, parityVectorList)
 *                         (include/normEncoder.h:44), host pointers, exact per-call semantics
 *   nfec_decode_vectors   NormDecoder::Decode(vectorList, numData, erasureCount, erasureLocs)
 *                         (include/normEncoder.h:53), host pointers, exact per-call semantics
 *   nfec_encode_segment_host / nfec_decode_vectors_host
 *                         the same two calls on the host CPU (GFNI / AVX2 region products)
 */
#ifndef NFEC_H
#define NFEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFEC_ABI_VERSION 1

/* codec families (NORM fec_id 5/2 -> RS8/RS16, fec_id 129 -> MDP; normSession.cpp:839-875) */
enum {
    NFEC_RS8 = 1,  /* GF(2^8) systematic Reed-Solomon, Rizzo Vandermonde generator   */
    NFEC_RS16 = 2, /* GF(2^16) systematic Reed-Solomon, native-endian 16-bit symbols */
    NFEC_MDP = 3   /* legacy GF(2^8) LFSR code (fec_id 129)                          */
};

/* status codes: >= 0 success */
enum {
    NFEC_OK = 0,
    NFEC_EINVAL = -1,   /* bad argument (sizes, alignment, null pointers)            */
    NFEC_ENOMEM = -2,   /* device or host allocation failed                            */
    NFEC_EDEVICE = -3,  /* HIP runtime/launch failure or no usable gfx950 device       */
    NFEC_ERANGE = -4,   /* numData + numParity exceeds the field (Init returns false)  */
    NFEC_ENOTSUP = -5   /* combination not supported (e.g. accumulate with MDP encode) */
};

/* batch flags */
enum {
    /* XOR results into the existing output bytes, exactly like the reference's
     * accumulate-into-caller-zeroed-buffer contract (Encode parity, Decode erased
     * source).  Without it outputs are overwritten, which is byte-identical whenever
     * the caller zeroed them first (NORM always does: normObject.cpp:1579, :2240-2252). */
    NFEC_ACCUMULATE = 1u << 0
};

typedef struct nfec_codec nfec_codec;

typedef struct nfec_codec_info {
    int32_t kind;         /* NFEC_RS8 / NFEC_RS16 / NFEC_MDP */
    int32_t device;       /* HIP device ordinal the codec lives on (-1: host-only codec) */
    uint32_t num_data;    /* k (ndata)  */
    uint32_t num_parity;  /* m (npar)   */
    uint32_t vector_size; /* bytes per segment vector processed (vectorSize given to Init) */
    uint32_t symbol_bytes;/* 1 (RS8/MDP) or 2 (RS16) */
} nfec_codec_info;

/*
 * A batch of FEC blocks resident in device memory (HBM).
 * Block b, segment slot s starts at  blocks + b*block_stride + s*seg_stride.
 * Slot layout per block mirrors NORM's block segment list (normSegment.h:79,
 * normObject.cpp:1610): slots [0, numData) hold source symbols, slots
 * [numData, numData + m) hold parity symbols.
 * Requirements: blocks, seg_stride and block_stride are multiples of 8 bytes
 * (NORM's segment pool is 8-byte aligned, normSegment.cpp:25-27), and
 * seg_stride >= vector_size.
 */
typedef struct nfec_block_batch {
    void* blocks;              /* device pointer */
    uint64_t block_stride;     /* bytes */
    uint32_t seg_stride;       /* bytes */
    uint32_t nblocks;
    const uint16_t* num_data;  /* device [nblocks] per-block numData (<= k), or NULL = k */
    uint32_t flags;            /* NFEC_ACCUMULATE */
    uint32_t reserved;
} nfec_block_batch;

/* ---- version / device ---- */
int nfec_abi_version(void);
/* SHA-256 (hex) of the sources this library was built from: the .cpp/.hip/.hpp/.h files of
 * norm_amd/csrc, then the .h files of include and include/norm_fec, each list sorted by path,
 * contents concatenated (norm_amd/Makefile). */
const char* nfec_build_id(void);
/* number of visible gfx950 devices (0 when none) */
int nfec_device_count(void);
/* human-readable message for the last error on this thread */
const char* nfec_last_error(void);

/* ---- host-only generator construction (no GPU needed) ----
 * Writes the m x k parity rows of the systematic generator (RS8/RS16: Rizzo Vandermonde
 * code, normEncoderRS8.cpp:428-450; MDP: the LFSR block map for k source symbols),
 * row-major, symbol_bytes per element.  Returns NFEC_ERANGE where Init would return false. */
int nfec_build_generator(int kind, uint32_t num_data, uint32_t num_parity, void* host_out, size_t bytes);

/* ---- codec lifecycle ---- */
int nfec_codec_create(int device, int kind, uint32_t num_data, uint32_t num_parity,
                      uint32_t vector_size, nfec_codec** out);

/* Codec options (nfec_codec_config.flags): correct alternatives of the RS16 kernels, chosen per
 * codec (the tests run both; the defaults are the faster ones), and a codec without a GPU. */
enum {
    NFEC_OPT_RS16_SHARED_TABLES = 1u << 0, /* RS16 products on the shared-LDS-table kernel
                                              instead of the tower-field one */
    NFEC_OPT_RS16_TOEPLITZ_OFF = 1u << 1,  /* RS16 encode never uses the Toeplitz split */
    NFEC_OPT_RS16_TOEPLITZ_ON = 1u << 2,   /* ... uses it whenever the shape allows it, not
                                              only where it needs fewer passes */
    NFEC_OPT_HOST_ONLY = 1u << 3,          /* no device at all (a NORM node without a usable
                                              gfx950): Init's math on the host, and only the host
                                              per-call paths (nfec_encode_segment_host,
                                              nfec_decode_vectors_host) run; every GPU entry
                                              returns NFEC_EDEVICE.  No device list. */
    NFEC_OPT_RS16_TOEPLITZ_ONE_LEVEL = 1u << 4  /* the Toeplitz split at one Karatsuba level at
                                                   most (default: two where they save passes) */
};

/* One codec over one or several GPUs of a node.  With several devices the codec holds the
 * generator on each (one full codec per device; a device may be listed twice, which gives two
 * independent pipelines on it) and stripes every host batch (nfec_*_host, nfec_*_host_vectors
 * and their async forms) over them in contiguous block ranges [i*B/N, (i+1)*B/N), one host
 * thread and one staging pipeline per device, no exchange between the ranges: the in-process
 * form of SURVEY 8e's block striping for single-process callers such as one NORM session
 * (normSession.cpp:834-889) or npc (normPrecode.cpp:588-880).  A device batch (nfec_encode /
 * nfec_decode) runs on the first listed device that holds it (NFEC_EINVAL when a device
 * allocation is on none of them; a batch in host-mapped or registered host memory runs on the
 * first device, as a one-device codec would take it);
 * per-call work (nfec_encode_segment / nfec_decode_vectors) on the first device. */
typedef struct nfec_codec_config {
    int32_t kind;             /* NFEC_RS8 / NFEC_RS16 / NFEC_MDP */
    uint32_t num_data, num_parity, vector_size;
    const int32_t* devices;   /* HIP device ordinals (NULL with num_devices 0: device 0) */
    uint32_t num_devices;     /* 0 or 1: one device; at most 64 */
    uint32_t flags;           /* NFEC_OPT_* */
} nfec_codec_config;
int nfec_codec_create_ex(const nfec_codec_config* config, nfec_codec** out);
/* Number of devices of a codec; their ordinals go to devices[0 .. min(n, cap)) when non-NULL. */
int nfec_codec_num_devices(const nfec_codec* codec, int32_t* devices, uint32_t cap);
void nfec_codec_destroy(nfec_codec* codec);
int nfec_codec_get_info(const nfec_codec* codec, nfec_codec_info* out);
/* Encode paths the codec chose at creation (bit mask, < 0 on error):
 *   NFEC_FEATURE_RS16_TOEPLITZ: unshortened, overwriting RS16 encodes use the Toeplitz split of
 *   the generator (three (m/2)-row products over k/2 columns). */
#define NFEC_FEATURE_RS16_TOEPLITZ 1
/* ... at two Karatsuba levels: nine (m/4)-row products over k/4 columns (tower kernel) */
#define NFEC_FEATURE_RS16_TOEPLITZ2 2
int nfec_codec_features(const nfec_codec* codec);
/* Device-batch encodes so far per path that took them (diagnostics: which kernel family a
 * batch shape reaches).  counts[i] for i < n; returns NFEC_PATH_COUNT (< 0 on error). */
#define NFEC_PATH_FIXED 0        /* bit-sliced kernels generated for the (k, m) generator (RS8, MDP; shortened RS8 too) */
#define NFEC_PATH_RUNTIME 1      /* bit-sliced, runtime coefficients (any RS8 / MDP shape) */
#define NFEC_PATH_RS16_SPLIT 2   /* RS16 Toeplitz split (shortened batches too, tower kernel) */
#define NFEC_PATH_RS16_PRODUCT 3 /* RS16 one product over all k columns (tower or shared-table kernel) */
#define NFEC_PATH_GENERIC 4      /* table-lookup kernels */
#define NFEC_PATH_COUNT 5
int nfec_codec_encode_paths(const nfec_codec* codec, uint64_t* counts, uint32_t n);
/* The same for device-batch decodes (NFEC_DPATH_*). */
#define NFEC_DPATH_FIXED 0        /* RS8 closed-form plan + fused / bit-sliced repair for the (k, m) generator (shortened too) */
#define NFEC_DPATH_RUNTIME 1      /* one-pass repair on the runtime-coefficient kernel (any RS8 shape, MDP) */
#define NFEC_DPATH_RS16_TOWER 2   /* RS16 closed-form plan, both stages on the tower kernel */
#define NFEC_DPATH_GENERIC 3      /* Gauss-Jordan plan and table-lookup kernels */
#define NFEC_DPATH_COUNT 4
int nfec_codec_decode_paths(const nfec_codec* codec, uint64_t* counts, uint32_t n);
/* Device batches so far whose last vec % 8 bytes ran on the tail kernels beside the fast kernels
 * (counts[0] encodes, counts[1] decodes); returns 2, < 0 on error. */
int nfec_codec_tail_batches(const nfec_codec* codec, uint64_t* counts, uint32_t n);
/* Copies the m x k parity rows of the systematic generator (row p = generator row k+p),
 * row-major, elements of symbol_bytes each.  MDP: the m x k matrix of the LFSR code for a
 * full block of k source symbols.  bytes must be >= m*k*symbol_bytes. */
int nfec_codec_get_generator(const nfec_codec* codec, void* host_out, size_t bytes);

/* ---- batched device-resident path (the performance path) ----
 * stream is a hipStream_t (NULL = legacy default stream).  Calls are asynchronous with
 * respect to the host; results are ready when the stream reaches them.  (A large RS16 encode on
 * the two-level Toeplitz split runs half of its sub-batches on a second stream of the codec's
 * own; that stream starts after the caller's stream and joins it before the call's end, so the
 * ordering the caller sees is the same.) */
int nfec_encode(nfec_codec* codec, const nfec_block_batch* batch, void* stream);

/* erasure_locs: device [nblocks][erasure_stride] sorted slot indices (source erasures
 * first, then missing parity, as NormObject builds them); erasure_counts: device
 * [nblocks]; status: device [nblocks] or NULL -- per block the reference Decode return
 * value (erasureCount on success, 0 when the block cannot be repaired).
 * Erased source slots are repaired; parity slots are never written.
 * A codec owns one decode workspace (like the reference decoder's scratch matrices,
 * normEncoderRS8.cpp:559-606): decode calls on one codec must be ordered (same stream, or
 * synchronised by the caller); encode calls only read the codec and may run concurrently. */
int nfec_decode(nfec_codec* codec, const nfec_block_batch* batch, const uint16_t* erasure_locs,
                uint32_t erasure_stride, const uint16_t* erasure_counts, int32_t* status,
                void* stream);

/* ---- receiver assembly on the device ----
 * What NormObject::HandleObjectMessage does between a NORM_DATA arrival and the Decode call
 * (normObject.cpp:1548-1644) for a receiver whose segments are already in HBM: put each received
 * segment into its (block, slot) of a device batch, keep NORM's per-block reception mask, and
 * build the erasure lists Decode takes from that mask.  Two ways in: nfec_rx_place takes (block,
 * symbol) per segment as the wire layer (nfec_payload_id_read, nfec_fti_read) gives them on the
 * host, and only those descriptors are uploaded; nfec_rx_ingest reads each message's FEC payload
 * ID from the wire buffer on the device and needs no host-built descriptor.  All device entries are
 * asynchronous on stream, like nfec_decode, and run on the codec device that holds the batch
 * (nfec_rx_erasures: the mask).
 *
 * A reception mask is uint32_t received[nblocks][mask_stride] in device memory, mask_stride >=
 * (k + m + 31) / 32: bit s % 32 of word s / 32 is set when slot s of the block holds a received
 * segment.  The caller zeroes it once.  Bits at or past numData_b + m are ignored everywhere. */
typedef struct nfec_rx_segments {
    const void*     payloads;     /* device: received payload bytes, any byte alignment      */
    const uint64_t* offsets;      /* device [count]: byte offset of segment i in payloads    */
    const uint32_t* block_index;  /* device [count]: block of the batch                      */
    const uint16_t* symbol_id;    /* device [count]: slot (source < numData_b <= parity)     */
    const uint16_t* length;       /* device [count]: payload bytes, <= vector_size           */
    uint32_t count;
} nfec_rx_segments;

/* Places segment i into block b = block_index[i], slot s = symbol_id[i] of the batch.  With
 * nd_b = batch->num_data ? num_data[b] : k, a segment is rejected when b >= nblocks, nd_b is
 * outside [1, k], s >= nd_b + m or length[i] > vector_size.  Otherwise the slot is claimed by one
 * atomic OR on its mask word: when the bit was set already the segment is a duplicate and is
 * dropped (NORM's IsPending test at the top of HandleObjectMessage, race-free: exactly one of
 * several copies, within one call or across calls, wins the slot); when it was clear the segment
 * is placed: the slot's first length[i] bytes become the payload, bytes [length[i], vector_size)
 * zero (the reference's zero pad of a short last or stream segment).  Bytes [vector_size,
 * seg_stride) of a slot are never written; a rejected or duplicate segment writes no slot and no
 * mask word.  stats (device [3], may be NULL; the caller zeroes it): the placed, duplicate and
 * rejected counts are added to stats[0..2].  batch->flags is ignored. */
int nfec_rx_place(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_segments* segments,
                  uint32_t* received, uint32_t mask_stride, uint32_t* stats, void* stream);

typedef struct nfec_rx_messages {      /* device arrays; offsets/length are nfec_tx_list's */
    const void*     payloads;          /* the wire buffer, any byte alignment                   */
    uint64_t        payload_bytes;     /* ... and its size                                      */
    const uint64_t* offsets;           /* [count]: byte offset of message i's payload; its
                                          payload ID is the idlen bytes in front of it          */
    const uint16_t* length;            /* [count]: payload bytes                                */
    uint32_t        count;
    const uint64_t* count_dev;         /* device, may be NULL: process min(count, *count_dev)   */
} nfec_rx_messages;

/* The receiver intake, nfec_tx_emit's mirror: reads message i's FEC payload ID from the wire
 * buffer and places its payload in the same pass.  With off = offsets[i], len = length[i] and
 * idlen = nfec_payload_id_length(fec_id):
 *   - NFEC_EINVAL for a fec_id / fec_m pair nfec_payload_id_read refuses, and for fec_id 0 (a
 *     message without an ID names no slot).
 *   - A message is unreadable when off < idlen or off + len > payload_bytes: it is rejected, its
 *     outputs are 0xFFFFFFFF / 0xFFFF, and no byte of it is loaded.
 *   - Otherwise the idlen bytes [off - idlen, off) are decoded exactly as nfec_payload_id_read
 *     decodes them (big-endian, at any byte alignment) into block_id, s and, for fec_id 129,
 *     block_len.  The block field has `bits` bits: 24 for fec_id 5 and fec_id 2 / fec_m 8, 16 for
 *     fec_id 2 / fec_m 16, 32 for fec_id 129.  The block of the batch is b = (block_id -
 *     first_block_id) mod 2^bits, the inverse of nfec_tx_emit's first_block_id + b after the ID's
 *     truncation: a window that wraps the block field works.
 *   - block_index_out[i] = b, even when b >= nblocks, and symbol_id_out[i] = s (device [count],
 *     each may be NULL).
 *   - From here on nfec_rx_place's rule with (b, s, len): rejected when b >= nblocks, nd_b is
 *     outside [1, k], s >= nd_b + m or len > vector_size, and for fec_id 129 also when block_len !=
 *     nd_b; otherwise the slot is claimed by one atomic OR on the reception mask, a duplicate is
 *     dropped without a write, and a placed message's len bytes go into the slot, zeros up to
 *     vector_size, nothing into [vector_size, seg_stride).
 *   - stats[0..2] (device, may be NULL; the caller zeroes it) are nfec_rx_place's counters:
 *     placed, duplicate, rejected.
 *   - Every load from the wire buffer is an aligned chunk of at most 16 bytes that holds at least
 *     one byte of [off - idlen, off + len), so no load leaves a page the message touches: the wire
 *     buffer may end at the end of an allocation.  A duplicate or a rejected message loads its ID
 *     chunk or chunks (two when the ID straddles a 16-byte boundary) and nothing else.
 * With count_dev given, min(count, *count_dev) messages are processed and the outputs past them keep
 * their bytes, so nfec_tx_list -> nfec_tx_emit -> nfec_rx_ingest chains on a stream: offsets and
 * length are the list's arrays, count_dev its block_start + 2 * nblocks.  Asynchronous on stream,
 * on the codec device that holds the batch; owns no codec state; batch->flags is ignored.  count ==
 * 0 or nblocks == 0 is NFEC_OK and launches nothing; null and stride checks as nfec_rx_place. */
int nfec_rx_ingest(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_messages* messages,
                   uint8_t fec_id, uint8_t fec_m, uint32_t first_block_id,
                   uint32_t* received, uint32_t mask_stride,
                   uint32_t* block_index_out, uint16_t* symbol_id_out,   /* device [count], may be NULL */
                   uint32_t* stats, void* stream);
/* The parse half of nfec_rx_ingest's rule on host arrays (wire: wire_bytes bytes of host memory):
 * no codec, no GPU.  For callers of the host-vector paths and of nfec_rx_place.  Fills
 * block_index_out / symbol_id_out / block_len_out ([count], each may be NULL; block_len is 0 where
 * the ID carries none); an unreadable message gets 0xFFFFFFFF / 0xFFFF / 0xFFFF.  Returns the number
 * of readable messages; NFEC_EINVAL for a refused fec_id / fec_m pair or a null wire, offsets or
 * length with count > 0, NFEC_ERANGE for a count above 2^31 - 1. */
int nfec_rx_parse_host(uint8_t fec_id, uint8_t fec_m, uint32_t first_block_id,
                       const void* wire, uint64_t wire_bytes, const uint64_t* offsets, const uint16_t* length,
                       uint32_t count, uint32_t* block_index_out, uint16_t* symbol_id_out, uint16_t* block_len_out);

/* The erasure lists nfec_decode takes, from reception masks, as NormObject builds them
 * (normObject.cpp:1560-1606): a block with no source slot of [0, nd_b) missing gets count 0 and
 * nothing listed (not even missing parity); otherwise every missing source slot ascending, then
 * every missing parity slot of [nd_b, nd_b + m) ascending.  erasure_counts[b] is the full number
 * even past erasure_stride (nfec_decode answers status 0 for it); only the first erasure_stride
 * entries are written.  A block whose nd_b is outside [1, k] gets count 0.  num_data: device
 * [nblocks] or NULL (= k). */
int nfec_rx_erasures(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride,
                     const uint16_t* num_data, uint32_t nblocks, uint16_t* erasure_locs,
                     uint32_t erasure_stride, uint16_t* erasure_counts, void* stream);
/* nfec_rx_erasures into lists the codec owns (stride m, part of the decode workspace: the
 * ordering rule of nfec_decode holds), then nfec_decode on them.  batch->flags and status as
 * nfec_decode; the mask is only read.  Counted by nfec_codec_decode_paths like nfec_decode. */
int nfec_decode_received(nfec_codec* codec, const nfec_block_batch* batch, const uint32_t* received,
                         uint32_t mask_stride, int32_t* status, void* stream);
/* nfec_rx_erasures' rule on host arrays, for callers of nfec_decode_host_vectors who hold NORM's
 * mask: no codec, no GPU.  NFEC_EINVAL for null arrays, k or m of 0, k + m > 65536 or a
 * mask_stride below (k + m + 31) / 32. */
int nfec_rx_erasures_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                          const uint16_t* num_data, uint32_t nblocks, uint16_t* erasure_locs,
                          uint32_t erasure_stride, uint16_t* erasure_counts);

/* ---- repair requests on the device ----
 * The step of the receiver's cycle that leads back to the sender's pending masks: the repair-request
 * content of a NORM_NACK from the reception masks in HBM, as NormObject::AppendRepairRequest builds it
 * with flush set and nacking_mode NACK_NORMAL (normObject.cpp:1179-1381) and, per block,
 * NormBlock::AppendRepairRequest (normSegment.cpp:524-630).  The caller bounds the call at the last
 * block the sender has finished; the max_pending_block / max_pending_segment form, the NACK's message
 * header, its timers and the back-off draw stay the caller's, as does what the sender does with a
 * NACK beyond handling it (hold-off, transmit index).  Whether the NACK is sent at all, suppression,
 * is nfec_rx_handle_repair_content / nfec_rx_repair_pending ("NACK suppression and repair
 * advertisements on the device").
 *
 * Per block, with nd_b = num_data ? num_data[b] : k and "pending" a clear bit of the reception mask
 * in [0, nd_b + m): e = pending source slots, p = received parity slots.  A block is
 *   absent  (class 2) when no bit of [0, nd_b + m) is set (the reference holds no NormBlock for it),
 *   needing (class 1) when it is not absent and e > p,
 *   silent  (class 0) otherwise: complete, decodable (0 < e <= p: what nfec_decode_received
 *           repairs), or nd_b outside [1, k].
 * A needing block asks for (normSegment.cpp:536-554): with e > m every pending slot of [0, nd_b + m)
 * except the first m pending ones, otherwise the pending slots of [nd_b, nd_b + e).  A maximal run
 * of consecutive requested slots is one unit (:562-621): a run of 1 or 2 is an ITEMS unit of one or
 * two items, a run of 3 or more a RANGES unit of two items, its first and last slot.  The units of a
 * needing block form one chain; its requests carry flag SEGMENT (0x01).
 * Across blocks (normObject.cpp:1207-1278) a maximal run of consecutive absent blocks is a unit of
 * the same three kinds, every item with symbol 0 and its own block's nd (a range: the first and the
 * last block's), flag BLOCK (0x02).  A chain of block-level units runs from one needing block (or
 * the start) to the next (or the end); silent blocks separate its units but do not end it.  Output
 * is in block order: a run's unit is emitted at the position of the run's last block, and a chain's
 * units stand before the needing block that ends it.
 * Walking a chain, a unit opens a new request when it is the chain's first, when its form differs
 * from the previous unit's, or when the open request holds max_units units already.  The last is a
 * bound the caller controls where the reference stops at a full NACK: with max_units at least the
 * longest same-form stretch the bytes are what the reference's calls append to an unbounded NACK.
 * A request is form (u8: ITEMS 1, RANGES 2), flags (u8), length of its items in bytes (u16,
 * big-endian), then the items (NormRepairRequest::Pack, normMessage.cpp:263-276); an item is fec_id
 * (u8), 0 (u8), object id (u16, big-endian), then the bytes nfec_payload_id_write writes for
 * (first_block_id + b, symbol, nd_b) (AppendRepairItem / AppendRepairRange, :163-235).  Everything
 * is a multiple of 4 bytes.  With NFEC_NACK_INFO every request also carries INFO (0x04), and when
 * nothing else was produced the content is the INFO-only request (normObject.cpp:1365-1372): ITEMS,
 * flags INFO, one item with block 0, block length 0, symbol 0. */
#define NFEC_NACK_INFO 1u   /* flags: the object's NORM_INFO is pending too */

/* content: device, 4-byte aligned, `capacity` bytes; bytes at or past capacity and bytes at or past
 * the total are not written.  block_start: device uint64 [nblocks + 1][2], the call's workspace and
 * an output: row b = {bytes emitted at positions before b, that is the offset of the first request
 * byte emitted at block b's position; block b's class 0 / 1 / 2}, row nblocks = {bytes, requests}.
 * totals: device uint64 [4] = {bytes, requests, needing blocks, absent blocks}, the full numbers even
 * past capacity (nfec_tx_list's rule).  Asynchronous on stream, on the codec device that holds the
 * mask; owns no codec state; the mask is only read.  NFEC_EINVAL for a fec_id / fec_m pair
 * nfec_payload_id_write refuses and for fec_id 0, for flags other than NFEC_NACK_INFO, for max_units
 * of 0 or above 65535 / (2 * item length) (item length = 4 + nfec_payload_id_length(fec_id)), for
 * null arrays, a content that is not 4-byte aligned and a mask_stride below (k + m + 31) / 32.
 * nblocks == 0 is NFEC_OK and writes zero totals. */
int nfec_rx_repair_requests(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride,
                            const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                            uint16_t object_id, uint32_t first_block_id, uint32_t flags, uint32_t max_units,
                            void* content, uint64_t capacity, uint64_t* block_start, uint64_t* totals,
                            void* stream);
/* nfec_rx_repair_requests' rule on host arrays: no codec, no GPU (content at any alignment).  Also
 * NFEC_EINVAL for k or m of 0 and k + m > 65536. */
int nfec_rx_repair_requests_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                                 const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                                 uint16_t object_id, uint32_t first_block_id, uint32_t flags,
                                 uint32_t max_units, void* content, uint64_t capacity, uint64_t* block_start,
                                 uint64_t* totals);
/* The parser of repair-request content, for the sender's side and for tests: NormRepairRequest::
 * Unpack (normMessage.cpp:279-305) and ::Iterator (:335-358) over content[0, bytes) in host memory.
 * Unit u < capacity gets unit_flags[u], unit_form[u] and first[u] / last[u] = {object id, block id
 * as on the wire, block length (fec_id 129; else 0), symbol}; every item of a request that is not
 * RANGES is a unit with first = last.  The arrays are [capacity] / [capacity][4] and may be NULL.
 * It stops at a header that does not fit or whose length exceeds what is left, at a RANGES request
 * with an odd item count, and at an item with a foreign fec_id (a range: either of its items); a
 * request's bytes behind its last whole item are skipped.  Returns the number of units read before
 * the stop, even past capacity; *consumed (may be NULL) = the offset of the header or item it
 * stopped at, or bytes.  NFEC_EINVAL for a refused fec_id / fec_m pair or a null content with bytes
 * > 0, NFEC_ERANGE for more than 2^31 - 1 units. */
int nfec_repair_parse_host(uint8_t fec_id, uint8_t fec_m, const void* content, uint64_t bytes,
                           uint8_t* unit_flags, uint8_t* unit_form, uint32_t* first, uint32_t* last,
                           uint32_t capacity, uint64_t* consumed);
/* The operator of the kernels' segmented scans on {value, flag} pairs, out = a then b (for the host
 * test of its associativity). */
void nfec_nack_scan_combine_host(const uint64_t a[2], const uint64_t b[2], uint64_t out[2]);

/* ---- sender assembly on the device ----
 * What NormObject::NextSenderMsg does once a block's parity exists (normObject.cpp:1877-2078) for
 * a sender whose blocks are in HBM: walk the blocks and their pending masks in order, pick each
 * segment's payload length, write the FEC payload ID in front of the payload and clear the
 * pending bit.  The mirror of the receiver section: nfec_tx_list's four arrays are the ones
 * nfec_rx_segments takes, so a loopback needs no conversion.  Device entries are asynchronous on
 * stream; nfec_tx_list runs on the codec device that holds the mask, nfec_tx_emit on the one that
 * holds the batch.  Neither owns codec state: calls may run concurrently with anything.
 *
 * A pending mask has the reception mask's layout: uint32_t pending[nblocks][mask_stride],
 * mask_stride >= (k + m + 31) / 32, bit s % 32 of word s / 32 is slot s.  The caller sets it as
 * NormBlock::TxInit does (normSegment.h:106-118: bits [0, numData + autoParity)) and as TxUpdate /
 * ActivateRepairs do (normSegment.cpp:261-339) from what nfec_repair_parse_host reads out of a
 * NACK, or lets nfec_tx_activate_repairs set it ("sender repair state on the device").  Bits at or
 * past numData_b + m are ignored.
 *
 * The transmission list.  With nd_b = num_data ? num_data[b] : k (device [nblocks] or NULL), the
 * entries are: blocks ascending, within a block the pending slots of [0, nd_b + m) ascending
 * (NextSenderMsg's first-pending-block / first-pending-segment walk, :1877, :1989); a block whose
 * nd_b is outside [1, k] lists nothing.  seg_length: device uint16 [nblocks][length_stride],
 * length_stride >= k, or NULL.  A source slot s < nd_b is listed with length seg_length[b][s], a
 * parity slot with the block's seg_size_max, the maximum of seg_length[b][0 .. nd_b) over all
 * source slots, pending or not (:2050, :2071); with seg_length NULL both are vector_size.  A
 * length above vector_size is listed as it is (nfec_tx_emit rejects it).  Offsets are packed
 * behind `gap` free bytes per message (room for the message header and the payload ID): entry i's
 * payload starts at (i + 1) * gap + the lengths of the entries before it.
 * block_start: device uint64 [nblocks + 1][2]; block_start[b] = {index of block b's first entry,
 * byte offset at which its first message's gap begins}, row nblocks = the totals {entries, bytes}.
 * The totals are the full numbers even past capacity; only the first `capacity` entries of the
 * four arrays are written (nfec_rx_erasures' rule for erasure_stride).  block_start is also the
 * call's only workspace. */
int nfec_tx_list(const nfec_codec* codec, const uint32_t* pending, uint32_t mask_stride,
                 const uint16_t* num_data, uint32_t nblocks, const uint16_t* seg_length,
                 uint32_t length_stride, uint32_t gap, uint64_t* offsets, uint32_t* block_index,
                 uint16_t* symbol_id, uint16_t* length, uint32_t capacity, uint64_t* block_start,
                 void* stream);
/* nfec_tx_list's rule on host arrays: no codec, no GPU.  NFEC_EINVAL for null arrays, k or m of 0,
 * k + m > 65536, a vector_size outside [1, 65535], a mask_stride below (k + m + 31) / 32 or a
 * length_stride below k. */
int nfec_tx_list_host(uint32_t k, uint32_t m, uint32_t vector_size, const uint32_t* pending,
                      uint32_t mask_stride, const uint16_t* num_data, uint32_t nblocks,
                      const uint16_t* seg_length, uint32_t length_stride, uint32_t gap,
                      uint64_t* offsets, uint32_t* block_index, uint16_t* symbol_id, uint16_t* length,
                      uint32_t capacity, uint64_t* block_start);

typedef struct nfec_tx_segments {      /* device arrays, as nfec_tx_list writes them */
    void* payloads;                    /* the wire buffer, any byte alignment           */
    uint64_t payload_bytes;            /* ... and its size                              */
    const uint64_t* offsets;           /* [count]: byte offset of entry i's payload     */
    const uint32_t* block_index;       /* [count]: block of the batch                   */
    const uint16_t* symbol_id;         /* [count]: slot                                 */
    const uint16_t* length;            /* [count]: payload bytes, <= vector_size        */
    uint32_t count;                    /* entries the arrays hold (upper bound)         */
    const uint64_t* count_dev;         /* device, may be NULL: process min(count, *count_dev)
                                          entries (block_start's total), so list -> emit
                                          chains on a stream without a synchronize       */
} nfec_tx_segments;

/* Entry i, with b = block_index[i], s = symbol_id[i], len = length[i], off = offsets[i] and idlen =
 * nfec_payload_id_length(fec_id) (0 for fec_id 0: no payload ID), writes the bytes [off - idlen,
 * off + len) of payloads: first what nfec_payload_id_write(fec_id, fec_m, first_block_id + b
 * (32-bit wrap), s, nd_b, ...) writes, then the first len bytes of slot s of block b.  No other
 * byte of payloads is written, or read and written back: the neighbouring message may share a
 * cache line.  No byte outside the slot's own seg_stride bytes is read.  With pending given (may
 * be NULL) the slot's bit is cleared by one atomic AND (UnsetPending, normObject.cpp:2075).
 * An entry is rejected, with no byte and no mask word written, when b >= nblocks, nd_b is outside
 * [1, k], s >= nd_b + m, len > vector_size, off < idlen or off + len > payload_bytes: a wrong
 * descriptor cannot make the call write outside the wire buffer or read outside the batch.
 * stats (device [2], may be NULL; the caller zeroes it): the emitted and rejected counts are
 * added to stats[0..1].  NFEC_EINVAL for a fec_id / fec_m pair nfec_payload_id_write refuses.
 * batch->flags is ignored; the batch is only read. */
int nfec_tx_emit(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_tx_segments* segments,
                 uint8_t fec_id, uint8_t fec_m, uint32_t first_block_id, uint32_t* pending,
                 uint32_t mask_stride, uint32_t* stats, void* stream);

/* ---- sender repair state on the device ----
 * The step that closes the cycle: from the repair-request content of the NACKs of one repair cycle
 * (the bytes nfec_rx_repair_requests writes, behind each NORM_NACK's own header) to the pending
 * masks nfec_tx_list reads, by NORM's repair economy: a sender that holds m parity segments answers
 * "e segments of block b are missing" with e fresh parity segments, aggregates over the receivers
 * of a cycle (the largest e is what gets sent) and retransmits named segments only once the parity
 * is used up.  In the reference: NormSession::SenderHandleNackMessage, the !holdoff arm
 * (normSession.cpp:3706-4300), NormBlock::HandleSegmentRequest (normSegment.cpp:341-402),
 * NormObject::HandleBlockRequest (normObject.cpp:352-385), NormSession::OnRepairTimeout
 * (normSession.cpp:4720-4750) with NormObject::TxReset / ActivateRepairs (normObject.cpp:388-537)
 * and NormBlock::TxReset (normSegment.cpp:219-259), and NextSenderMsg's end of block
 * (normObject.cpp:2079-2083, ResetParityCount).  The call chain of a repair cycle is
 *   nfec_tx_handle_nacks x N -> nfec_tx_activate_repairs -> nfec_tx_list -> nfec_tx_emit ->
 *   nfec_tx_end_blocks.
 * Every block of the batch counts as held by the sender: it has a NormBlock and its parity exists
 * (the situation after nfec_encode).  Out of scope: the hold-off arm (TxUpdate against the transmit
 * index), several objects per call, SenderRecoverBlock, the stream's LockBlocks / LockSegments,
 * squelch, timers and CC feedback.  The content of NORM_CMD(REPAIR_ADV) is nfec_tx_repair_adv
 * ("NACK suppression and repair advertisements on the device").
 *
 * The state: caller-allocated arrays, device memory for the device entries, host memory for the
 * *_host entries.  repair has the pending mask's layout.  TxInit is parity = {auto_parity, 0},
 * everything else zero; TxRecover is parity = {m, m} (normSegment.h:106-129). */
#define NFEC_TX_REPAIR_OBJECT 1u   /* an OBJECT-level request named the object (tx_repair_mask) */
#define NFEC_TX_REPAIR_INFO   2u   /* repair_info                                                */
#define NFEC_TX_PENDING_INFO  4u   /* pending_info, set by activation                            */
typedef struct nfec_tx_repair_state {
    uint32_t* repair;        /* [nblocks][mask_stride]: NormBlock::repair_mask                    */
    uint16_t* parity;        /* [nblocks][2]: {parity_offset, parity_count}                       */
    uint32_t* block_repair;  /* [(nblocks + 31) / 32]: NormObject::repair_mask, one bit per block */
    uint32_t* object;        /* [1]: NFEC_TX_REPAIR_OBJECT | NFEC_TX_REPAIR_INFO | NFEC_TX_PENDING_INFO */
} nfec_tx_repair_state;

/* SenderHandleNackMessage, !holdoff, for one object.  Message i of nacks is the repair-request
 * content payloads[offsets[i], offsets[i] + length[i]) of one NORM_NACK, at any byte alignment;
 * count_dev is honoured.  A message that does not lie inside payload_bytes is unreadable: it is
 * counted and no byte of it is loaded.  Every load is an aligned chunk of at most 16 bytes that
 * holds at least one byte of the message (nfec_rx_ingest's rule).
 *
 * Order is part of the rule: the messages are handled in index order and each message's requests
 * and items in their order in the bytes; the call behaves exactly as if one thread did that.
 *
 * A message is parsed as nfec_repair_parse_host parses it.  Where the parser stops the message
 * ends: the units before the stop stand and the message is counted as cut short (a message whose
 * last request is followed by fewer than 4 bytes is cut short too).  The level of a request comes
 * from its flags in the reference's order (normSession.cpp:3763-3784): SEGMENT (0x01), else BLOCK
 * (0x02), else OBJECT (0x08), else INFO (0x04); a request with none of them is skipped (its units
 * are counted as ignored and change nothing, not even the stretch below).  A unit is (first,
 * last); in an ITEMS request last = first.  The block of the batch of an item is (block id -
 * first_block_id) mod 2^bits, as in nfec_rx_ingest.
 *   - Foreign object.  A SEGMENT- or BLOCK-level unit whose first item names another object id is
 *     ignored (the squelch is the caller's).  An OBJECT- or INFO-level unit is of this object when
 *     (object_id - first.obj) mod 2^16 <= (last.obj - first.obj) mod 2^16, else foreign.
 *   - INFO flag.  A unit of this object in a request that carries INFO sets NFEC_TX_REPAIR_INFO.
 *     (A stated simplification: the reference looks at the first unit of an object's stretch only;
 *     receivers put the flag on every request or on none.)
 *   - OBJECT level sets NFEC_TX_REPAIR_OBJECT; INFO level does nothing beyond the INFO flag.
 *   - BLOCK level (HandleBlockRequest): with b0, b1 the blocks of first and last, sets the
 *     block_repair bits of [b0, min(b1, nblocks - 1)]; nothing when b0 > b1 or b0 >= nblocks.
 *   - SEGMENT level, block b of first (last's block is not looked at, as in the reference).  The
 *     unit is not applied when b >= nblocks, when nd_b is outside [1, k], when last.symbol <
 *     first.symbol (the reference would add a wrapped count; no receiver sends it), or when the
 *     unit is fresh and b's block_repair bit is set at that moment (IsRepairSet, :4048).  A unit
 *     is fresh unless the previous SEGMENT-level unit of this message was applied and was for the
 *     same block; a foreign unit of any level in between also makes the next one fresh
 *     (freshObject), BLOCK-, OBJECT- and INFO-level units of this object in between do not.  A
 *     unit that continues a stretch is not tested against block_repair again.  An applied unit's
 *     erasure count is E = extra_parity + the widths (last.symbol - first.symbol + 1) of the
 *     applied units of its stretch up to and including itself, in 32 bits.  It then runs
 *     NormBlock::HandleSegmentRequest(first.symbol, last.symbol, nd_b, m, E) (normSegment.cpp:
 *     341-402) on the block's parity pair {o, c} and repair mask:
 *       first.symbol < nd_b:  o = c = m, and the slots [first, last] are set;
 *       else, with avail = m - o:
 *         E <= avail:  when E > c the slots [nd_b + o + c, nd_b + o + E) are set and c = E;
 *         E >  avail:  when c < avail the slots [nd_b + o + c, nd_b + m) are set, c = avail and
 *                      first += avail; then the slots [first, last] are set (the branch the
 *                      reference marks "TBD").
 *     Bits at or past nd_b + m are never set.
 * unit_capacity bounds the units of the call (totals[0]); workspace is device memory, 16-byte
 * aligned, of at least nfec_tx_nack_workspace_bytes(unit_capacity, count, nblocks) bytes.  When the
 * call's units exceed unit_capacity no state is changed and totals = {units, 0, 0, 0, cut short,
 * unreadable}: the caller repeats the call with more room.  Otherwise totals (device uint64 [6]) =
 * {units in all, SEGMENT units applied, SEGMENT units not applied plus units ignored (foreign, or
 * of a request without a level), block_repair bits newly set, messages cut short, messages
 * unreadable}.  The result does not depend on the order in which the device's atomics land.
 *
 * Asynchronous on stream, on the codec device that holds state->repair; owns no codec state.  The
 * pending mask is not an argument: handling never touches it.  NFEC_EINVAL for a fec_id / fec_m pair
 * nfec_payload_id_read refuses and for fec_id 0, for null arrays, a mask_stride below (k + m + 31)
 * / 32, a workspace that is null, misaligned or below the query's size, and extra_parity > 65535.
 * count == 0 or nblocks == 0 is NFEC_OK with zero totals. */
int nfec_tx_handle_nacks(const nfec_codec* codec, const nfec_rx_messages* nacks, uint8_t fec_id, uint8_t fec_m,
                         uint16_t object_id, uint32_t first_block_id, const uint16_t* num_data, uint32_t nblocks,
                         uint32_t mask_stride, uint32_t extra_parity, const nfec_tx_repair_state* state,
                         uint32_t unit_capacity, void* workspace, uint64_t workspace_bytes,
                         uint64_t* totals /* device [6] */, void* stream);
/* (count does not enter the size today; pass nacks->count) */
uint64_t nfec_tx_nack_workspace_bytes(uint32_t unit_capacity, uint32_t count, uint32_t nblocks);
/* nfec_tx_handle_nacks' rule on host arrays (nacks' arrays, num_data, state and totals in host
 * memory): no codec, no GPU, no workspace.  Also NFEC_EINVAL for k or m of 0 and k + m > 65536. */
int nfec_tx_handle_nacks_host(uint32_t k, uint32_t m, const nfec_rx_messages* nacks, uint8_t fec_id, uint8_t fec_m,
                              uint16_t object_id, uint32_t first_block_id, const uint16_t* num_data,
                              uint32_t nblocks, uint32_t mask_stride, uint32_t extra_parity,
                              const nfec_tx_repair_state* state, uint32_t unit_capacity, uint64_t* totals);

/* OnRepairTimeout for the object (normSession.cpp:4720-4750): what the handled NACKs of a cycle
 * left in the state goes into the pending mask.  Block TxReset (normSegment.cpp:219-259): the
 * block's repair bits of [0, nd_b + m) become zero in every case; when pending over [0, nd_b + m)
 * differs from the bits [0, nd_b + auto_parity), pending over [0, nd_b + m) becomes exactly those
 * bits and parity becomes {auto_parity, m} (a reset "with a change").
 *   With NFEC_TX_REPAIR_OBJECT set (NormObject::TxReset): every block is TxReset; nothing else of
 *   the blocks' repair masks is activated.
 *   Otherwise (NormObject::ActivateRepairs): every block whose block_repair bit is set is TxReset;
 *   then for every block pending |= repair and repair = 0, over [0, nd_b + m).
 * In both cases block_repair is cleared, and in the object word NFEC_TX_REPAIR_INFO moves to
 * NFEC_TX_PENDING_INFO, NFEC_TX_REPAIR_OBJECT is cleared, and NFEC_TX_PENDING_INFO is also set when
 * any block's TxReset changed something (NormObject::TxReset sets pending_info only when the object
 * has NORM_INFO or the FTI travels in it, normObject.cpp:418-424: the caller masks the bit where
 * neither holds).  Blocks with nd_b outside [1, k] are left alone.  totals (device uint64 [3]) =
 * {blocks reset with a change, blocks whose segment repairs were activated, pending bits over all
 * blocks after the call}.  Asynchronous on stream, on the codec device that holds pending.
 * NFEC_EINVAL for null arrays, auto_parity > m and a mask_stride below (k + m + 31) / 32; nblocks ==
 * 0 is NFEC_OK with zero totals and leaves the state alone. */
int nfec_tx_activate_repairs(const nfec_codec* codec, const uint16_t* num_data, uint32_t nblocks, uint32_t auto_parity,
                             uint32_t* pending, uint32_t mask_stride, const nfec_tx_repair_state* state,
                             uint64_t* totals /* device [3] */, void* stream);
int nfec_tx_activate_repairs_host(uint32_t k, uint32_t m, const uint16_t* num_data, uint32_t nblocks,
                                  uint32_t auto_parity, uint32_t* pending, uint32_t mask_stride,
                                  const nfec_tx_repair_state* state, uint64_t* totals);

/* NextSenderMsg's end of block (normObject.cpp:2079-2083, ResetParityCount): for every block whose
 * pending mask over [0, nd_b + m) is empty, parity_offset = min(parity_offset + parity_count, m)
 * and parity_count = 0: the parity sent in this cycle is no longer fresh.  Idempotent.  The caller
 * runs it after an emission (nfec_tx_emit with its pending argument) and before the next
 * nfec_tx_handle_nacks; between a handle call and its activation it would be wrong, because the
 * repairs handled so far count on the parity_count it clears.  Only state->parity is used and
 * written.  Blocks with nd_b outside [1, k] are left alone.  Asynchronous on stream. */
int nfec_tx_end_blocks(const nfec_codec* codec, const uint16_t* num_data, uint32_t nblocks, const uint32_t* pending,
                       uint32_t mask_stride, const nfec_tx_repair_state* state, void* stream);
int nfec_tx_end_blocks_host(uint32_t k, uint32_t m, const uint16_t* num_data, uint32_t nblocks,
                            const uint32_t* pending, uint32_t mask_stride, const nfec_tx_repair_state* state);

/* ---- NACK suppression and repair advertisements on the device ----
 * What makes the repair cycle a multicast one: during its back-off a receiver listens to the NACKs of
 * the others and to the sender's NORM_CMD(REPAIR_ADV), and stays silent when what it needs has been
 * asked for already; the sender advertises what it is about to repair.  In the reference:
 * NormSenderNode::HandleRepairContent (normNode.cpp:1069-1187), called for overheard NACKs
 * (:1060-1062) and for REPAIR_ADV (:906-911); NormObject::SetRepairs / SetRepairInfo
 * (normObject.h:274-279) and NormBlock::SetRepairs (normSegment.h:216-222); the decision at the end
 * of the back-off, NormSenderNode::OnRepairTimeout (normNode.cpp:2362-2390), NormObject::
 * IsRepairPending(flush) (normObject.cpp:1137-1177) and NormBlock::IsRepairPending
 * (normSegment.cpp:174-216); on the sender NormSession::SenderBuildRepairAdv (normSession.cpp:
 * 4598-4708), NormObject::AppendRepairAdv (normObject.cpp:540-683) and NormBlock::AppendRepairAdv
 * (normSegment.cpp:405-493).  A receiver's round is
 *   zero the state -> nfec_rx_handle_repair_content x N -> nfec_rx_repair_pending ->
 *   nfec_rx_repair_requests when it sends,
 * the sender's
 *   nfec_tx_handle_nacks x N -> nfec_tx_repair_adv -> nfec_tx_activate_repairs -> ...
 * One object per call, flush form only (nfec_rx_repair_requests' and nfec_tx_handle_nacks' limits).
 * Out of scope: timers and the back-off draw, the non-flush form bounded by current_block_id, the
 * NORM_REPAIR_ADV_FLAG_LIMIT flag of a full advertisement, and CC feedback.
 *
 * The receiver's suppression state: caller-allocated arrays, device memory for the device entries,
 * host memory for the *_host entries; the mask layouts are the reception mask's.  The caller zeroes
 * all three at the start of a NACK cycle: that is the whole of the reset NormObject::
 * ReceiverRepairCheck makes when it starts the repair timer (normObject.cpp:1098-1110), so no entry
 * exists for it. */
#define NFEC_RX_REPAIR_OBJECT 1u   /* rx_repair_mask names the object */
#define NFEC_RX_REPAIR_INFO   2u   /* NormObject::repair_info          */
typedef struct nfec_rx_repair_state {
    uint32_t* repair;        /* [nblocks][mask_stride]: the receiver's NormBlock::repair_mask */
    uint32_t* block_repair;  /* [(nblocks + 31) / 32]: NormObject::repair_mask               */
    uint32_t* object;        /* [1]: NFEC_RX_REPAIR_OBJECT | NFEC_RX_REPAIR_INFO              */
} nfec_rx_repair_state;

/* HandleRepairContent for one object.  Message i of messages is the repair-request content of one
 * overheard NORM_NACK or of one NORM_CMD(REPAIR_ADV), at any byte alignment; count_dev is honoured.
 * Unreadable messages, the loads (aligned chunks of at most 16 bytes that hold a byte of the
 * message), the parser, where a message is cut short, a request's level, the own / foreign test of
 * a unit and the block of the batch of an item are nfec_tx_handle_nacks'.  Per unit of this object:
 *   - INFO level sets NFEC_RX_REPAIR_INFO.
 *   - OBJECT level sets NFEC_RX_REPAIR_OBJECT; the request's INFO flag is not looked at (:1141-1146).
 *   - BLOCK level sets NFEC_RX_REPAIR_INFO when the request carries INFO, and the block_repair bits
 *     of [b0, min(b1, nblocks - 1)]; nothing when b0 > b1 or b0 >= nblocks.
 *   - SEGMENT level, block b of the first item, sets NFEC_RX_REPAIR_INFO when the request carries
 *     INFO, applied or not (SetRepairInfo stands in front of FindBlock, :1172).  The unit is applied
 *     when b < nblocks, nd_b lies in [1, k], last.symbol >= first.symbol and block b is held: it is a
 *     needing block (class 1) by nfec_rx_repair_requests' classification of `received` at the time
 *     of the call.  (The reference has a NormBlock for exactly these: an absent block has none, a
 *     complete or decodable one was decoded and released.)  An applied unit sets the repair bits
 *     [first.symbol, last.symbol], clipped at nd_b + m.
 * Every update is an OR: the result depends neither on the order of the messages, nor on how they
 * are split over calls, nor on the order in which the device's atomics land (the reference's
 * freshObject / freshBlock are lookup caches).  There is no workspace and no capacity.  totals
 * (device uint64 [6]) = {units in all, SEGMENT units applied, SEGMENT units not applied plus units
 * ignored (foreign, or of a request without a level), block_repair bits newly set, messages cut
 * short, messages unreadable}; the newly-set count is exact however many messages name a block.
 * `received` is only read.  Asynchronous on stream, on the codec device that holds state->repair;
 * owns no codec state.  NFEC_EINVAL for a fec_id / fec_m pair nfec_payload_id_read refuses and for
 * fec_id 0, for null arrays and a mask_stride below (k + m + 31) / 32.  count == 0 or nblocks == 0
 * is NFEC_OK with zero totals. */
int nfec_rx_handle_repair_content(const nfec_codec* codec, const nfec_rx_messages* messages, uint8_t fec_id,
                                  uint8_t fec_m, uint16_t object_id, uint32_t first_block_id,
                                  const uint32_t* received, uint32_t mask_stride, const uint16_t* num_data,
                                  uint32_t nblocks, const nfec_rx_repair_state* state,
                                  uint64_t* totals /* device [6] */, void* stream);
/* nfec_rx_handle_repair_content's rule on host arrays: no codec, no GPU.  Also NFEC_EINVAL for k or
 * m of 0 and k + m > 65536. */
int nfec_rx_handle_repair_content_host(uint32_t k, uint32_t m, const nfec_rx_messages* messages, uint8_t fec_id,
                                       uint8_t fec_m, uint16_t object_id, uint32_t first_block_id,
                                       const uint32_t* received, uint32_t mask_stride, const uint16_t* num_data,
                                       uint32_t nblocks, const nfec_rx_repair_state* state, uint64_t* totals);

/* The decision at the end of the back-off, flush form: does the receiver send a NACK for the object?
 * Per block, with the class and the requested slots of nfec_rx_repair_requests: a silent block is
 * not pending; an absent block is pending unless its block_repair bit is set; a needing block is
 * pending unless its block_repair bit is set or every requested slot has its repair bit set
 * (NormBlock::IsRepairPending: the slots it presets are exactly the pending slots the request does
 * not name).  The object is suppressed when NFEC_RX_REPAIR_OBJECT is set; otherwise it sends when
 * flags holds NFEC_NACK_INFO (the object's NORM_INFO is pending) and NFEC_RX_REPAIR_INFO is clear,
 * or when any block is pending.  The state is only read: the reference destroys its masks here
 * (XCopy), this call does not.  pending_blocks: device uint32 [(nblocks + 31) / 32], may be NULL:
 * bit b % 32 of word b / 32 is set when block b is pending; every word is written, bits at or past
 * nblocks are zero, the caller need not zero it.  totals (device uint64 [4]) = {send: 0 or 1,
 * blocks pending, needing blocks suppressed, absent blocks suppressed}; the three block counts are
 * the full numbers whatever the object word says.  Asynchronous on stream, on the codec device that
 * holds the mask.  NFEC_EINVAL for flags other than NFEC_NACK_INFO, null arrays and a mask_stride
 * below (k + m + 31) / 32.  nblocks == 0 is NFEC_OK with zero totals and reads no state. */
int nfec_rx_repair_pending(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride,
                           const uint16_t* num_data, uint32_t nblocks, const nfec_rx_repair_state* state,
                           uint32_t flags, uint32_t* pending_blocks, uint64_t* totals /* device [4] */,
                           void* stream);
int nfec_rx_repair_pending_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                                const uint16_t* num_data, uint32_t nblocks, const nfec_rx_repair_state* state,
                                uint32_t flags, uint32_t* pending_blocks, uint64_t* totals);

/* The repair-request content of a NORM_CMD(REPAIR_ADV) from the sender's repair state as it stands
 * after nfec_tx_handle_nacks and before nfec_tx_activate_repairs.  The arguments and outputs are
 * nfec_rx_repair_requests' with the state in place of the reception mask (mask_stride is
 * state->repair's; only repair, block_repair and object are read) and without flags: INFO is
 * NFEC_TX_REPAIR_INFO, read from the object word on the device.  Per block: nd_b outside [1, k] is
 * silent; a set block_repair bit makes a whole block (class 2, what an absent block is to a NACK);
 * else any repair bit in [0, nd_b + m) makes class 1 with those bits as the requested slots; else
 * silent.  From there the runs, units, chains and requests are those of "repair requests on the
 * device", word for word: NormObject::AppendRepairAdv is the walk of AppendRepairRequest over
 * another mask, and one set of kernels runs both.  totals = {bytes, requests, blocks with segment
 * requests, whole blocks}; block_start's second column holds the classes.
 * With NFEC_TX_REPAIR_OBJECT set the content is one request and nothing of the blocks
 * (normSession.cpp:4681): form ITEMS, flags OBJECT (INFO is not added: SenderBuildRepairAdv's
 * request never carries it), one item {object id, block 0, block length k, symbol 0}; every row of
 * block_start is {0, 0} and totals = {bytes, 1, 0, 0}.  A quirk of the reference that is not
 * reproduced: its loop emits this request only when another object follows in the table (:4622
 * tests NULL != nextObject), so the last object's is lost; a caller that wants that drops the
 * content.  NFEC_EINVAL as nfec_rx_repair_requests, and for null state arrays; nblocks == 0 is
 * NFEC_OK with zero totals and reads no state. */
int nfec_tx_repair_adv(const nfec_codec* codec, const nfec_tx_repair_state* state, uint32_t mask_stride,
                       const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                       uint16_t object_id, uint32_t first_block_id, uint32_t max_units, void* content,
                       uint64_t capacity, uint64_t* block_start, uint64_t* totals, void* stream);
int nfec_tx_repair_adv_host(uint32_t k, uint32_t m, const nfec_tx_repair_state* state, uint32_t mask_stride,
                            const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                            uint16_t object_id, uint32_t first_block_id, uint32_t max_units, void* content,
                            uint64_t capacity, uint64_t* block_start, uint64_t* totals);

/* ---- NORM_DATA messages on the device ----
 * nfec_tx_emit and nfec_rx_ingest move payloads and their FEC payload IDs; the host fills and reads
 * the rest of every header.  This pair moves whole NORM_DATA messages: the sender call writes the
 * message header, the payload ID, the header extension and the payload, the receiver call takes raw
 * datagrams by (offset, length) alone, classifies them by NormMsg::InitFromBuffer's rule (reference
 * src/common/normMessage.cpp:17-92), finds the ID and the payload where the header says they are
 * and places the payload in the same pass.  It is the layout the reference's default sender uses:
 * fti_mode FTI_ALWAYS (src/common/normSession.cpp:58) puts the FTI extension between the ID and the
 * payload of every NORM_DATA (src/common/normObject.cpp:1808-1857).
 *
 * A message on the wire (include/normMessage.h:688-696, :769-779, :1183-1186; big-endian fields):
 *   byte 0          version << 4 | type: version 1, type DATA = 2
 *   byte 1          hdr_len, the header's length in 32-bit words
 *   bytes 2-3       sequence
 *   bytes 4-7       source_id
 *   bytes 8-9       instance_id
 *   byte 10         grtt                      byte 11    backoff << 4 | gsize
 *   byte 12         flags                     byte 13    fec_id
 *   bytes 14-15     object transport id
 *   bytes 16 ...    the FEC payload ID (nfec_payload_id_write's bytes: 4, or 8 for fec_id 129)
 *   ... 4 hdr_len   header extensions; a sender attaches the FTI alone (nfec_fti_write's bytes)
 *   4 hdr_len ...   the payload
 * so a header is 20 / 20 / 24 bytes for fec_id 5 / 2 / 129 and 32 / 36 / 40 with the FTI. */
typedef struct nfec_data_header {      /* the fields one call's messages share */
    uint32_t source_id;                /* SendMessage: local_node_id (normSession.cpp:5013) */
    uint16_t instance_id;              /* :4923 */
    uint16_t first_sequence;           /* message i carries first_sequence + i mod 2^16 (:4924) */
    uint8_t  grtt, backoff, gsize;     /* quantised, as the session holds them (:1329-1331);
                                          backoff and gsize are 4-bit fields */
    uint8_t  flags;                    /* NormObjectMsg::Flag bits, written as given */
    uint8_t  fec_id, fec_m;
    uint16_t object_id;
    uint8_t  ext[16]; uint8_t ext_bytes;   /* 0, or an FTI extension as nfec_fti_write wrote it
                                              (12 bytes for fec_id 5, 16 for 2 and 129) */
} nfec_data_header;

/* 16 + nfec_payload_id_length(fec_id) + ext_bytes: the header's bytes, and the `gap` to give
 * nfec_tx_list.  NFEC_EINVAL for a fec_id other than 2, 5 and 129 and for an ext_bytes that is
 * neither 0 nor the FTI's length for that fec_id. */
int nfec_data_header_bytes(uint8_t fec_id, uint8_t ext_bytes);

/* nfec_tx_emit with the whole NORM_DATA header in front of the payload.  segments: nfec_tx_list's
 * arrays built with gap = H = nfec_data_header_bytes(header->fec_id, header->ext_bytes).  Entry i,
 * with b, s, len and off as in nfec_tx_emit, writes exactly the bytes [off - H, off + len) of
 * payloads: the header above with sequence first_sequence + i, hdr_len H / 4 and the payload ID of
 * (first_block_id + b, s, nd_b), header->ext where ext_bytes > 0, then the slot's first len bytes.
 * Everything else is nfec_tx_emit's rule: no other byte of payloads is written, or read and written
 * back; no byte outside the slot's seg_stride is read; with pending given the slot's bit is cleared
 * by one atomic AND; count_dev bounds the entries.  An entry is rejected, with no byte and no mask
 * word written, when b >= nblocks, nd_b is outside [1, k], s >= nd_b + m, len > vector_size, off <
 * H, off + len > payload_bytes or len + H > 65535.  stats (device [2], may be NULL): emitted,
 * rejected.  msg_offsets_out / msg_length_out (device [count], each may be NULL): off - H and len +
 * H of entry i, the datagram table a NIC or nfec_rx_ingest_data takes; a rejected entry gets 0 / 0
 * (a datagram nfec_rx_ingest_data finds unreadable).  NFEC_EINVAL for a fec_id / fec_m pair
 * nfec_payload_id_write refuses, for a backoff or gsize above 15 and for an ext_bytes
 * nfec_data_header_bytes refuses; the batch is only read. */
int nfec_tx_emit_data(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_tx_segments* segments,
                      const nfec_data_header* header, uint32_t first_block_id, uint32_t* pending,
                      uint32_t mask_stride, uint64_t* msg_offsets_out, uint16_t* msg_length_out,
                      uint32_t* stats, void* stream);

typedef struct nfec_data_filter {      /* the sender, code and object one receiver call takes */
    uint32_t source_id;
    uint16_t instance_id;
    uint8_t  fec_id, fec_m;
    uint16_t object_id;
} nfec_data_filter;

enum {                                 /* a datagram's class: the first whose condition holds */
    NFEC_DGRAM_UNREADABLE = 0,         /* off + length > payload_bytes or length < 8: no byte loaded */
    NFEC_DGRAM_OTHER_TYPE = 1,         /* not NORM_DATA: INFO / CMD / NACK / ACK / REPORT are the host's */
    NFEC_DGRAM_MALFORMED = 2,          /* InitFromBuffer fails: length < 16 + idlen(byte 13), an unknown
                                          fec_id byte, 4 hdr_len < 16 + idlen or 4 hdr_len > length */
    NFEC_DGRAM_OTHER_SENDER = 3,       /* source_id or instance_id is not the filter's */
    NFEC_DGRAM_OTHER_CODE = 4,         /* the fec_id byte is not the filter's */
    NFEC_DGRAM_OTHER_OBJECT = 5,       /* the object id is not the filter's */
    NFEC_DGRAM_REJECTED = 6,           /* from here on nfec_rx_ingest's rule */
    NFEC_DGRAM_DUPLICATE = 7,
    NFEC_DGRAM_PLACED = 8,
    NFEC_DGRAM_CLASSES = 9,
    NFEC_DGRAM_PARSED = 9              /* nfec_rx_parse_data_host only: past the filter */
};

/* The receiver intake for raw datagrams.  datagrams->offsets[i] / length[i] are the start and the
 * length of datagram i in the wire buffer (not of its payload); count_dev as in nfec_rx_ingest.
 * Each datagram gets one class, above.  For one past the filter the payload ID is read at byte 16
 * as nfec_rx_ingest reads it, b = (block_id - first_block_id) mod 2^bits, the payload is the bytes
 * [4 hdr_len, length) (none is a payload of length 0), and nfec_rx_ingest's rule applies: the fec_id
 * 129 block-length check, one atomic OR for the claim, the payload zero-padded to vector_size and
 * nothing written into [vector_size, seg_stride).
 *   - class_out[i] (device uint8 [count], may be NULL): the class.
 *   - sequence_out[i] (device [count], may be NULL): bytes 2-3, for every readable datagram: the
 *     host's loss estimator input.
 *   - block_index_out / symbol_id_out: as in nfec_rx_ingest for a datagram past the filter, all
 *     ones for any other.
 *   - stats (device [9], may be NULL; the caller zeroes it): one counter per class, added once per
 *     wave.
 *   - totals (device uint64 [1], may be NULL; the caller sets totals[0] to all ones): totals[0]
 *     becomes the smallest i of a datagram past the filter whose first extension has type 64 (FTI)
 *     and lies inside the header: the host reads it there (at byte 16 + idlen of the datagram) with
 *     nfec_fti_read to size a new object.  Only the first extension is examined, and one whose
 *     length byte is 0 or that runs past 4 hdr_len is not an FTI.
 *   - Every load from the wire buffer is an aligned chunk of at most 16 bytes that holds at least
 *     one byte of [off, off + length); a datagram that is not placed loads the chunks of its first
 *     min(length, 28) bytes and nothing else.
 * filter->fec_id / fec_m: NFEC_EINVAL for a pair nfec_payload_id_read refuses.  Asynchronous on
 * stream, on the codec device that holds the batch; owns no codec state; count == 0 or nblocks == 0
 * launches nothing; null and stride checks as nfec_rx_ingest. */
int nfec_rx_ingest_data(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_messages* datagrams,
                        const nfec_data_filter* filter, uint32_t first_block_id, uint32_t* received,
                        uint32_t mask_stride, uint8_t* class_out, uint16_t* sequence_out,
                        uint32_t* block_index_out, uint16_t* symbol_id_out, uint32_t* stats, uint64_t* totals,
                        void* stream);

/* Host twins: no GPU, no codec; the header words and the parse are the kernels' own code.
 * nfec_data_header_write_host writes the header of message i of a call (sequence first_sequence +
 * i) for (block_id, symbol, block_len) into out and returns its length; NFEC_EINVAL as
 * nfec_tx_emit_data, and for a cap below the length. */
int nfec_data_header_write_host(const nfec_data_header* header, uint32_t i, uint32_t block_id, uint16_t symbol,
                                uint16_t block_len, void* out, size_t cap);
/* nfec_rx_ingest_data's parse on host arrays (wire: wire_bytes bytes of host memory).  class_out is
 * never PLACED, DUPLICATE or REJECTED: a datagram past the filter is NFEC_DGRAM_PARSED, and
 * nfec_rx_place's rule (with block_len_out for fec_id 129) decides the rest.  For such a datagram
 * payload_offset_out[i] = off + 4 hdr_len and payload_length_out[i] = length - 4 hdr_len, the
 * arrays nfec_rx_place and the host-vector paths take; for any other 0 / 0, and block / symbol /
 * block_len all ones.  sequence_out[i] is written for a readable datagram.  *fti_index_out: the
 * smallest i with an FTI as first extension, all ones when there is none.  Every output may be
 * NULL.  Reads no byte outside [off, off + length) of a datagram.  Returns the number of PARSED
 * datagrams; NFEC_EINVAL and NFEC_ERANGE as nfec_rx_parse_host. */
int nfec_rx_parse_data_host(const nfec_data_filter* filter, uint32_t first_block_id, const void* wire,
                            uint64_t wire_bytes, const uint64_t* offsets, const uint16_t* length, uint32_t count,
                            uint8_t* class_out, uint16_t* sequence_out, uint32_t* block_index_out,
                            uint16_t* symbol_id_out, uint16_t* block_len_out, uint64_t* payload_offset_out,
                            uint16_t* payload_length_out, uint64_t* fti_index_out);
/* The wire-buffer offsets of the aligned 16-byte chunks nfec_rx_ingest_data loads of a datagram at
 * (off, length) before it knows its class (chunk_out[3]); returns how many (0 for length < 8). */
int nfec_rx_data_chunks_host(uint64_t off, uint16_t length, uint64_t* chunk_out);

/* ---- NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the device ----
 * nfec_rx_repair_requests and nfec_tx_repair_adv produce repair-request content, nfec_tx_handle_nacks
 * and nfec_rx_handle_repair_content consume it.  These calls are the messages in between: a
 * receiver's content cut into NORM_NACK messages of at most segment_size content bytes each, the
 * sender's content behind a NORM_CMD(REPAIR_ADV) header, and on the far side the intake that tells
 * NACKs and advertisements from everything else in a receive buffer and finds their content.  With
 * them "reception masks -> NACKs on the wire -> sender repair state" and "sender state -> REPAIR_ADV
 * on the wire -> receiver suppression state" run on one stream without a synchronize.
 *
 * NORM_NACK on the wire (include/normMessage.h:1906-1989; big-endian fields), 24-byte base header:
 *   byte 0          version << 4 | type = 0x14      byte 1    hdr_len in 32-bit words
 *   bytes 2-3       sequence
 *   bytes 4-7       source_id (the receiver)
 *   bytes 8-11      sender_id
 *   bytes 12-13     instance_id                     bytes 14-15   reserved, 0
 *   bytes 16-19     grtt_response seconds           bytes 20-23   grtt_response microseconds
 *   ... 4 hdr_len   an optional header extension
 *   4 hdr_len ...   the repair-request content
 * NORM_CMD(REPAIR_ADV) (:1200-1249, :1688-1737), 16-byte base header:
 *   byte 0          0x13                            byte 1    hdr_len
 *   bytes 2-3       sequence
 *   bytes 4-7       source_id
 *   bytes 8-9       instance_id
 *   byte 10         grtt                            byte 11   backoff << 4 | gsize
 *   byte 12         flavor = 5                      byte 13   flags (NORM_REPAIR_ADV_FLAG_LIMIT = 1)
 *   bytes 14-15     reserved, 0
 *   then the extension and the content as in the NACK.
 * The only extension a sender of either message attaches is the 12-byte CC-feedback extension
 * (NormCCFeedbackExtension, :1741-1807); the caller supplies it as opaque bytes. */
typedef struct nfec_nack_header {      /* the fields one call's NACKs share */
    uint32_t source_id;                /* the receiver: local_node_id (normSession.cpp:5013) */
    uint32_t sender_id;                /* the sender the NACK is for */
    uint16_t instance_id;              /* the sender's instance */
    uint16_t first_sequence;           /* message i carries first_sequence + i * sequence_step */
    uint16_t sequence_step;            /* 0: every NACK carries first_sequence, as the reference
                                          sends all of them with 0 (normSession.cpp:4958) */
    uint32_t grtt_response_sec;        /* the sender's send time as the receiver echoes it */
    uint32_t grtt_response_usec;
    uint8_t  ext[12]; uint8_t ext_bytes;   /* 0, or a 12-byte CC-feedback extension */
} nfec_nack_header;

typedef struct nfec_adv_header {       /* the header of one NORM_CMD(REPAIR_ADV) */
    uint32_t source_id;                /* the sender */
    uint16_t instance_id;
    uint16_t sequence;
    uint8_t  grtt, backoff, gsize;     /* quantised, as the session holds them; backoff and gsize
                                          are 4-bit fields */
    uint8_t  ext[12]; uint8_t ext_bytes;   /* 0, or a 12-byte CC-feedback extension */
} nfec_adv_header;

/* 24 + ext_bytes and 16 + ext_bytes; NFEC_EINVAL for an ext_bytes other than 0 and 12. */
int nfec_nack_header_bytes(uint8_t ext_bytes);
int nfec_adv_header_bytes(uint8_t ext_bytes);

/* The cut rule: NormSenderNode::FragmentNack (src/common/normNode.cpp:2676-2772), which turns content
 * that exceeds one message into several (OnRepairTimeout, :2601-2610), with two departures.  With S =
 * segment_size, L = 4 + nfec_payload_id_length(fec_id) the item length, U the unit length of a
 * request (2 L for form RANGES, L for any other), P the content bytes in the open message and len a
 * request's length (4 + its item bytes), for each request in order:
 *   A. P + len <= S: the request is copied whole.
 *   B. otherwise, if the request has at least one unit and P + 4 + U <= S, it is split: a copy of its
 *      4-byte header (form, flags, and the length of the units that follow it in this message), then
 *      units while they fit; whenever the next unit does not fit (P + U > S) the message is closed and
 *      a new one opens with another copy of the header (P = 4).  The message that holds the request's
 *      last unit stays open.
 *   C. otherwise the message is closed, P = 0, and the same request is examined again.
 * Departure 1: in arm C the reference advances past the request it could not place and never sends
 * it (:2699-2702, :2756-2762).  Departure 2: the reference enters arm B on P + 4 < S alone and so can
 * end a message with a request header that has no items.  Where neither situation occurs the bytes
 * are the reference's; where everything fits, the one message is the content itself.
 * The walk stops at a request header that does not fit, at a length that runs past the content, at
 * item bytes that are not a multiple of L and at a RANGES request with an odd item count; what
 * precedes the stop stands.  (Items are not examined: a foreign fec_id, at which
 * nfec_repair_parse_host stops, is the consumer's to refuse.)  A request without items is legal: it
 * is copied when it fits, else arm C applies.
 * NFEC_EINVAL for a segment_size that is not a multiple of 4, below 4 + 2 L (the reference's loop
 * would not advance) or with segment_size + header bytes > 65535.
 *
 * nfec_nack_fragment writes whole NORM_NACK messages.  content: device, 4-byte aligned; the call
 * reads min(content_capacity, *content_bytes_dev) bytes of it, content_bytes_dev (device) being
 * totals[0] of the producing nfec_rx_repair_requests as it lies in HBM.  Message i is at wire + i *
 * pitch (wire: device, 4-byte aligned, wire_bytes bytes; pitch a multiple of 4, at least H +
 * segment_size with H = nfec_nack_header_bytes(header->ext_bytes)): the header with sequence
 * first_sequence + i * sequence_step, then its content by the rule above.  msg_offsets_out[i] = i *
 * pitch and msg_length_out[i] (device [capacity], each may be NULL) are the datagram table.  Only
 * the first min(capacity, wire_bytes / pitch) messages are written; no byte of wire outside a
 * message's own [i * pitch, i * pitch + length_i) is stored, or read and written back.
 * totals: device uint64 [6] = {messages, content bytes written (the messages' lengths without their
 * headers), requests read, requests split by arm B, content bytes consumed, 1 if cut short: the walk
 * stopped before the end of the content, or *content_bytes_dev exceeds content_capacity}: the full
 * numbers even past capacity.  totals[0] is what a consumer's nfec_rx_messages.count_dev points at.
 * block_start (device, may be NULL with nblocks 0) is the array the producing call wrote for the same
 * content: by that call's rule the bytes emitted at a needing block's position begin a chain and so
 * a request, and what follows them begins another, so offset 0 and both ends of every class-1 row are
 * request boundaries and the request headers between two of them are walked by one lane each.
 * Without the hint the call is correct but one lane walks every request header of the content: slow
 * (about 100 ms for 140,000 requests, measured; more than cutting on the host costs).  Every load is bounds-checked against the content
 * length: a hint that does not belong to the content yields unspecified messages but no access
 * outside the buffers.  workspace: device, 8-byte aligned, at least nfec_nack_fragment_workspace_bytes(
 * content_capacity, nblocks) bytes, the call's until it has run.  NFEC_ERANGE for a content_capacity
 * of 2^32 or more.  Asynchronous on stream, on the codec device that holds the content; owns no codec
 * state; the content is only read. */
int nfec_nack_fragment(const nfec_codec* codec, const void* content, uint64_t content_capacity,
                       const uint64_t* content_bytes_dev, const uint64_t* block_start, uint32_t nblocks,
                       uint8_t fec_id, uint32_t segment_size, const nfec_nack_header* header, void* wire,
                       uint64_t wire_bytes, uint32_t pitch, uint64_t* msg_offsets_out, uint16_t* msg_length_out,
                       uint32_t capacity, uint64_t* totals, void* workspace, uint64_t workspace_bytes,
                       void* stream);
uint64_t nfec_nack_fragment_workspace_bytes(uint64_t content_capacity, uint32_t nblocks);

/* One NORM_CMD(REPAIR_ADV) at wire (device, 4-byte aligned, wire_bytes >= H + segment_size with H =
 * nfec_adv_header_bytes(header->ext_bytes)): the header, then the first message of the same cut of
 * content (nfec_tx_repair_adv's, content_bytes_dev its totals[0]).  The flags byte has
 * NORM_REPAIR_ADV_FLAG_LIMIT set exactly when content remained; the reference leaves the flag "TBD"
 * (normSession.cpp:4646) and silently truncates.  Where everything fits the bytes are the
 * reference's.  msg_length_out (device uint16 [1]): the message's length, 0 for empty content, of
 * which nothing is written.  totals: device uint64 [3] = {content bytes written, content bytes left
 * out, limit flag}.  One wave walks the request headers of the first message (at most segment_size /
 * 4).  Asynchronous on stream; owns no codec state. */
int nfec_tx_repair_adv_message(const nfec_codec* codec, const void* content, uint64_t content_capacity,
                               const uint64_t* content_bytes_dev, uint8_t fec_id, uint32_t segment_size,
                               const nfec_adv_header* header, void* wire, uint64_t wire_bytes,
                               uint16_t* msg_length_out, uint64_t* totals, void* stream);

#define NFEC_CTL_ANY_INSTANCE 1u   /* filter flags: do not test instance_id (the reference's sender
                                      tests the id alone, normSession.cpp:2964) */
#define NFEC_CTL_TAKE_NACK    2u   /* give NACKs content entries (a sender's intake) */
#define NFEC_CTL_TAKE_ADV     4u   /* give REPAIR_ADVs content entries (a receiver's intake) */
typedef struct nfec_ctl_filter {
    uint32_t sender_id;                /* NACK: its sender_id field; CMD: its source_id */
    uint16_t instance_id;
    uint32_t local_id;                 /* messages from this node are its own; 0: no such test */
    uint32_t flags;                    /* NFEC_CTL_* */
} nfec_ctl_filter;

enum {                                 /* a control datagram's class: the first whose condition holds */
    NFEC_CTL_UNREADABLE = 0,           /* as NFEC_DGRAM_UNREADABLE: no byte loaded */
    NFEC_CTL_OTHER_TYPE = 1,           /* neither NORM_NACK (4) nor NORM_CMD (3) */
    NFEC_CTL_MALFORMED = 2,            /* InitFromBuffer fails (normMessage.cpp:17-92): length or 4 hdr_len
                                          below 24 (NACK) / 16 (CMD), or 4 hdr_len > length */
    NFEC_CTL_OTHER_FLAVOR = 3,         /* a CMD that is not REPAIR_ADV (5) */
    NFEC_CTL_OWN = 4,                  /* source_id == local_id (normSession.cpp:2816-2817) */
    NFEC_CTL_OTHER_SENDER = 5,         /* NACK: sender_id, CMD: source_id is not the filter's */
    NFEC_CTL_OTHER_INSTANCE = 6,       /* instance_id is not the filter's (not under ANY_INSTANCE) */
    NFEC_CTL_NACK = 7,
    NFEC_CTL_REPAIR_ADV = 8,
    NFEC_CTL_CLASSES = 9,
    NFEC_CTL_EXTENDED = 0x80           /* class_out's top bit (classes 7 and 8): 4 hdr_len exceeds the
                                          base header, an extension is there for the host to read */
};

/* The intake for control datagrams: datagrams as in nfec_rx_ingest_data.  Each gets one class,
 * above.  For a NACK under NFEC_CTL_TAKE_NACK and a REPAIR_ADV under NFEC_CTL_TAKE_ADV
 * content_offset_out[i] = off + 4 hdr_len and content_length_out[i] = length - 4 hdr_len; every
 * other datagram gets 0 / 0, which is a readable, empty message to nfec_tx_handle_nacks and
 * nfec_rx_handle_repair_content: the tables are index-aligned with the datagrams, so arrival order,
 * which nfec_tx_handle_nacks depends on, is kept, and they go into an nfec_rx_messages as they are.
 * class_out (device uint8 [count]), source_id_out (device uint32 [count]: bytes 4-7 of a readable
 * datagram, 0 for an unreadable one) and grtt_response_out (device uint32 [count][2]: seconds, microseconds of a NACK; 0 / 0
 * for any other) may be NULL; content_offset_out (uint64 [count]) and content_length_out (uint16
 * [count]) may not.  stats (device uint32 [9], may be NULL; the caller zeroes it): one counter per
 * class.  A CC extension is left in place for the host.  Every load from the wire buffer is an
 * aligned chunk of at most 16 bytes that holds at least one byte of the datagram's first min(length,
 * 24) bytes.  Outputs past min(count, *count_dev) keep their bytes.  Asynchronous on stream, on the
 * codec device that holds the wire buffer; owns no codec state; count == 0 launches nothing. */
int nfec_rx_ingest_control(const nfec_codec* codec, const nfec_rx_messages* datagrams, const nfec_ctl_filter* filter,
                           uint8_t* class_out, uint64_t* content_offset_out, uint16_t* content_length_out,
                           uint32_t* source_id_out, uint32_t* grtt_response_out, uint32_t* stats, void* stream);

/* Host twins: no GPU, no codec; the cut, the header words and the parse are the kernels' own code
 * (content and wire in host memory at any alignment).
 * nfec_nack_fragment_host: nfec_nack_fragment on host arrays, `bytes` the content's length.
 * nfec_nack_header_write_host: the header of message i of a call into out; returns its length.
 * nfec_adv_message_host: nfec_tx_repair_adv_message; returns the message's length.
 * nfec_ctl_parse_host: nfec_rx_ingest_control's outputs, stats included (added to); reads no byte
 * outside a datagram's first min(length, 24) bytes; returns the number of datagrams that got a
 * content entry. */
int nfec_nack_fragment_host(const void* content, uint64_t bytes, uint8_t fec_id, uint32_t segment_size,
                            const nfec_nack_header* header, void* wire, uint64_t wire_bytes, uint32_t pitch,
                            uint64_t* msg_offsets_out, uint16_t* msg_length_out, uint32_t capacity, uint64_t* totals);
int nfec_nack_header_write_host(const nfec_nack_header* header, uint32_t i, void* out, size_t cap);
int nfec_adv_message_host(const void* content, uint64_t bytes, uint8_t fec_id, uint32_t segment_size,
                          const nfec_adv_header* header, void* wire, uint64_t wire_bytes, uint64_t* totals);
int nfec_ctl_parse_host(const nfec_ctl_filter* filter, const void* wire, uint64_t wire_bytes, const uint64_t* offsets,
                        const uint16_t* length, uint32_t count, uint8_t* class_out, uint64_t* content_offset_out,
                        uint16_t* content_length_out, uint32_t* source_id_out, uint32_t* grtt_response_out,
                        uint32_t* stats);

/* ---- object segmentation on the device ----
 * The mapping between a NORM data object (a contiguous run of bytes) and the source slots of its
 * FEC blocks: one step before nfec_encode on the sender, one step after nfec_decode_received on
 * the receiver.  In the reference it is NormObject::Open's block partition
 * (src/common/normObject.cpp:134-137, :203-231; NORM spec 5.1.1, the RFC 5052 large / small
 * blocks), NormDataObject::ReadSegment (:2673-2718) with the zero pad of CalculateBlockParity
 * (:2203-2229) on the sender, and NormDataObject::WriteSegment (:2628-2670) on the receiver, which
 * is called for every received source segment (:1529) and for every repaired one after a
 * successful Decode (:1616).  Non-stream objects only: the entries take no object type
 * (NORM_OBJECT_STREAM has the next section's).
 *
 * The partition.  num_segments = ceil(object_size / segment_size) and num_blocks =
 * ceil(num_segments / num_data) (NormObjectSize's divide rounds up everywhere); large_block_size =
 * ceil(num_segments / num_blocks).  When num_segments == num_blocks * large_block_size every block
 * has that size and the layout says so the way the reference does: large_block_count = 0,
 * small_block_size = large_block_size, small_block_count = num_blocks.  Otherwise small_block_size
 * = large_block_size - 1, large_block_count = num_segments - num_blocks * small_block_size and
 * small_block_count = num_blocks - large_block_count.  Block b holds
 * b < large_block_count ? large_block_size : small_block_size segments (GetBlockSize); the large
 * blocks come first.  final_block_id = num_blocks - 1, and final_segment_size = object_size -
 * (num_segments - 1) * segment_size is the length of its last segment. */
typedef struct nfec_object_layout {
    uint64_t object_size;        /* bytes */
    uint32_t segment_size;       /* bytes of object per source segment */
    uint32_t num_data;           /* k the object was opened with */
    uint64_t num_segments;       /* ceil(object_size / segment_size) */
    uint32_t num_blocks;         /* ceil(num_segments / num_data) */
    uint32_t large_block_size, large_block_count;
    uint32_t small_block_size, small_block_count;
    uint32_t final_block_id, final_segment_size;
} nfec_object_layout;

/* Open's arithmetic.  Host only: no GPU, no codec.  NFEC_EINVAL for a null out, for object_size,
 * segment_size or num_data of 0, segment_size > 65535 or num_data > 65535; NFEC_ERANGE when
 * num_blocks does not fit 32 bits (Open refuses the object, :145). */
int nfec_object_layout_for(uint64_t object_size, uint32_t segment_size, uint32_t num_data,
                           nfec_object_layout* out);
/* ReadSegment's / WriteSegment's rule for segment `segment` of block `block`: its byte offset in
 * the object, large_block_size * segment_size * block + segment_size * segment below
 * large_block_count and large_block_size * segment_size * large_block_count + small_block_size *
 * segment_size * (block - large_block_count) + segment_size * segment from it on, and its length,
 * segment_size except final_segment_size for the last segment of final_block_id.  Either output
 * may be NULL.  NFEC_ERANGE for a block or a segment outside the object.  Host only. */
int nfec_object_segment(const nfec_object_layout* layout, uint32_t block, uint32_t segment,
                        uint64_t* offset, uint32_t* length);
/* num_data_out[i] = the size of block first_block + i, i < nblocks (host array): the num_data[]
 * of a batch that holds those blocks.  NFEC_ERANGE when first_block + nblocks > num_blocks. */
int nfec_object_block_sizes(const nfec_object_layout* layout, uint32_t first_block, uint32_t nblocks,
                            uint16_t* num_data_out);

/* The two device entries.  Batch block i is object block first_block + i and nd_i its size by the
 * layout; batch->num_data and batch->flags are ignored.  object (device memory, object_bytes of
 * it) may have any byte alignment; the batch obeys the usual 8-byte rules.  Both calls are
 * asynchronous on stream, run on the codec device that holds the batch, touch no codec state and
 * may run concurrently with anything.  NFEC_EINVAL for a null pointer (except the optional
 * arguments named below), layout->num_data != k, segment_size > vector_size, first_block +
 * nblocks > num_blocks, a mask_stride below (k + m + 31) / 32 when received is given, a
 * length_stride below k when seg_length_out is given, or object and batch in device memory of
 * different devices.  nblocks == 0 is NFEC_OK and launches nothing.
 *
 * nfec_object_read (sender): for every s < nd_i, with (off, len) from nfec_object_segment's rule,
 * the slot's bytes [0, len) become object[off, off + len) and its bytes [len, vector_size) zero
 * (CalculateBlockParity's pad; for segment_size + 8 == vector_size it covers the 8 bytes NORM
 * reserves for the stream payload header).  Bytes [vector_size, seg_stride) of a slot and the
 * slots [nd_i, k + m) are never written, and the object is only read: in aligned 16-byte chunks
 * that each hold at least one byte of it, so no load leaves a page the object touches.
 * num_data_out (device [nblocks], may be NULL): num_data_out[i] = nd_i.  seg_length_out (device
 * [nblocks][length_stride], may be NULL): seg_length_out[i][s] = len for s < nd_i; entries at or
 * past nd_i are not written.  These are the arrays nfec_encode (batch.num_data) and nfec_tx_list
 * take.  NFEC_EINVAL unless object_bytes >= object_size (ReadSegment would return 0 and fail the
 * block).
 *
 * nfec_object_write (receiver): segment (i, s), s < nd_i, is written when received is NULL, or
 * its bit is set in received[i] (the reception mask's layout), or status is given and status[i] >
 * 0 (nfec_decode's status of a repaired block): received source segments are delivered, erased
 * ones only after a successful Decode.  A written segment stores the first len' bytes of its slot
 * to object[off, off + len'), len' being len clamped at object_bytes as WriteSegment clamps at
 * data_max (:2664-2667): nothing at all when off >= object_bytes.  No other byte of the object is
 * written, or read and written back: the neighbouring segment, which shares 16-byte pieces and
 * cache lines, may be unselected, hold an earlier call's bytes or be written by another wave at
 * the same time.  No byte outside a slot's own seg_stride bytes is read; the batch and the mask
 * are only read.  stats (device [2], may be NULL; the caller zeroes it): the selected and the
 * not-selected segment counts are added to stats[0..1] (a selected segment wholly past
 * object_bytes counts as selected, as WriteSegment returns true for it). */
int nfec_object_read(const nfec_codec* codec, const nfec_object_layout* layout, const void* object,
                     uint64_t object_bytes, uint32_t first_block, const nfec_block_batch* batch,
                     uint16_t* num_data_out, uint16_t* seg_length_out, uint32_t length_stride,
                     void* stream);
int nfec_object_write(const nfec_codec* codec, const nfec_object_layout* layout, void* object,
                      uint64_t object_bytes, uint32_t first_block, const nfec_block_batch* batch,
                      const uint32_t* received, uint32_t mask_stride, const int32_t* status,
                      uint32_t* stats, void* stream);

/* ---- stream objects on the device ----
 * NORM's third object kind, NORM_OBJECT_STREAM: the reason every codec has vector_size =
 * segment_size + 8.  A stream segment is the 8-byte stream payload header (include/normMessage.h:
 * 1145-1196: payload_len, 2 bytes big-endian, at byte 0; payload_msg_start, 2 BE, at 2;
 * payload_offset, 4 BE, at 4) and up to segment_size bytes of the stream from byte 8 on.  The
 * three steps of NormStreamObject for a caller whose stream bytes are in HBM: frame (which bytes
 * make which segment: NormStreamObject::Write, src/common/normObject.cpp:4039-4232, the loop body
 * :4166-4210), pack (the segments into the source slots of a batch, one step before nfec_encode)
 * and unpack (repaired blocks back to the byte stream, one step after nfec_decode_received; what
 * NormStreamObject::ReadPrivate, :3700-3860, reads out of its segments).
 *
 * The framing rule.  A call frames n application writes (write_len[i], write_flags[i]) that lie
 * one behind the other in the stream; NFEC_STREAM_EOM: the write ends a message (Write's eom),
 * NFEC_STREAM_FLUSH: the flush mode of the write was not FLUSH_NONE.  The call's byte run is the
 * carry -- the state's carry_bytes bytes of the open trailing segment the calls before left --
 * followed by the writes; position 0 is its first byte, S = segment_size.  Cuts: position 0 and
 * the end position of every FLUSH write (coinciding cuts are one).  Between consecutive cuts a < b
 * lie ceil((b - a) / S) segments, segment j being [a + j S, min(a + (j + 1) S, b)); behind the
 * last cut only the full segments are closed, the rest (fewer than S bytes) is the new carry and
 * is not emitted.  No empty segment is emitted (:4198-4199: a flush closes a segment only when it
 * holds a byte).  A write is a message start when its length is not 0 and it is the stream's
 * first such write (:2788, msg_start(true)) or an EOM write lies between the nonzero write before
 * it and it, that write included (:4175-4180, :4214-4217: a zero-length EOM write raises the flag
 * too, and a zero-length write never takes it).  The header of segment [s, e): payload_len = e -
 * s; payload_msg_start = p - s + 1 for the first message-start position p in [s, e), else 0;
 * payload_offset = write_offset + s (mod 2^32), write_offset being the stream offset of position
 * 0.  Segment i of a call goes to slot q = first_slot + i of the stream: block q / k, slot q % k of
 * a batch whose block 0 is the block of slot 0 (stream blocks are always k wide, :2779). */
#define NFEC_STREAM_EOM   1u   /* write_flags: the write ends a message                         */
#define NFEC_STREAM_FLUSH 2u   /* write_flags: flush mode other than FLUSH_NONE                 */
#define NFEC_STREAM_END   1u   /* nfec_stream_pack flags: append Terminate's control segment    */

typedef struct nfec_stream_state {     /* a fresh stream: {0, 1, 0, 0, 0} (:2788, :2798)        */
    uint32_t write_offset;       /* stream offset of the carry's first byte; wraps at 2^32      */
    uint32_t msg_start_pending;  /* Write's msg_start flag: the next nonzero write starts a message */
    uint32_t carry_bytes;        /* bytes of the open trailing segment, < segment_size          */
    uint32_t carry_msg_start;    /* 0, or 1 + the position of the carry's first message start   */
    uint64_t next_slot;          /* segments closed so far: the next call's first_slot          */
} nfec_stream_state;

/* The rule on host arrays: no codec, no GPU.  seg_start[i] (byte offset of segment i's first byte
 * in the call's byte run, the carry included), seg_len[i] and seg_msg_start[i] hold `capacity`
 * entries; totals[4] = {segments, bytes consumed (the position at which the new carry begins: the
 * next call's byte run starts there), carry bytes, carry_msg_start}.  The totals are the full
 * numbers even past capacity; only the first `capacity` entries are written (nfec_tx_list's
 * rule).  *state is advanced (write_offset by the bytes consumed, next_slot by the segments), so
 * that framing the same writes in one call, or split over several calls at any write boundary,
 * gives the same segments.  NFEC_EINVAL for a null state or totals, null write arrays with n > 0,
 * null output arrays with capacity > 0, a segment_size outside [1, 65535 - 8], or a state with
 * carry_bytes >= segment_size or carry_msg_start > carry_bytes. */
int nfec_stream_frame_host(uint32_t segment_size, const uint32_t* write_len, const uint8_t* write_flags,
                           uint32_t n, nfec_stream_state* state, uint64_t* seg_start, uint16_t* seg_len,
                           uint16_t* seg_msg_start, uint32_t capacity, uint64_t* totals);

/* The same on device arrays, asynchronously on stream, on the codec device that holds totals; it
 * owns no codec state.  The state comes by value; the advanced state is written to *state_out
 * (device) and totals is a device uint64[4], so nfec_stream_pack (count_dev = totals) and the
 * caller's next step chain on them without a synchronize.  workspace: device, 8-byte aligned,
 * NFEC_STREAM_FRAME_WORKSPACE(n, capacity) bytes, the call's only workspace (five 64-bit words
 * per write: its scans).  Errors as the host entry's, plus a null workspace or state_out. */
#define NFEC_STREAM_FRAME_WORKSPACE(n, capacity) (((uint64_t)(n) + 2u) * 40u)
int nfec_stream_frame(const nfec_codec* codec, uint32_t segment_size, const uint32_t* write_len,
                      const uint8_t* write_flags, uint32_t n, nfec_stream_state state,
                      nfec_stream_state* state_out, uint64_t* seg_start, uint16_t* seg_len,
                      uint16_t* seg_msg_start, uint32_t capacity, uint64_t* totals, void* workspace,
                      void* stream);

typedef struct nfec_stream_segments {  /* device arrays, as nfec_stream_frame writes them       */
    const void* bytes;                 /* the call's byte run, any byte alignment               */
    uint64_t stream_bytes;             /* ... and its size                                      */
    const uint64_t* seg_start;         /* [count]                                               */
    const uint16_t* seg_len;           /* [count]                                               */
    const uint16_t* seg_msg_start;     /* [count]                                               */
    uint32_t count;                    /* entries the arrays hold (upper bound)                 */
    const uint64_t* count_dev;         /* device, may be NULL: process min(count, *count_dev)
                                          entries (totals[0] of nfec_stream_frame)              */
} nfec_stream_segments;

/* The two copy entries.  Both are asynchronous on stream, run on the codec device that holds the
 * batch, own no codec state, ignore batch->flags, and may run concurrently with anything
 * (nfec_stream_pack ignores batch->num_data too: it writes num_data_out).  NFEC_EINVAL for a null pointer (except the optional arguments named below),
 * unless 1 <= segment_size and segment_size + 8 <= vector_size, a length_stride below k when
 * seg_length_out is given, an out_stride below k when a per-slot output is given, a mask_stride
 * below (k + m + 31) / 32 when received is given, or stream bytes / window and batch in device
 * memory of different devices.  A call with nothing to do (no block, or no entry and no
 * NFEC_STREAM_END) is NFEC_OK and launches nothing.
 *
 * nfec_stream_pack (sender): entry i (start = seg_start[i], len = seg_len[i], ms =
 * seg_msg_start[i]) goes to slot q = first_slot + i: block q / k of the batch, slot q % k.  The
 * slot's bytes [0, 8) become the header {len, ms, write_offset + start}, its bytes [8, 8 + len)
 * bytes[start, start + len) and its bytes [8 + len, vector_size) zero.  Nothing is written in
 * [vector_size, seg_stride); the slot is never read; the stream bytes are only read, in aligned
 * 16-byte chunks that each hold a byte of the segment.  An entry is rejected and counted, with no
 * store, when len > segment_size, len == 0, start + len > stream_bytes or its block is >= nblocks
 * (it keeps its slot number): a wrong table cannot make the call read outside the stream bytes or
 * write outside the batch.  With NFEC_STREAM_END in flags the control segment of
 * NormStreamObject::Terminate (:3904-3995) follows the last entry, at slot first_slot + (entries
 * processed): length 0, msg_start 0, offset = write_offset + start + len of the last entry
 * processed, or write_offset when there is none -- the stream offset behind the last emitted
 * byte, as Terminate's Flush leaves write_offset (the caller frames its last write with FLUSH,
 * so that nothing is carried).  seg_length_out (device [nblocks][length_stride], may be NULL):
 * seg_length_out[b][s] = 8 + len for every slot the call fills (ReadSegment's return,
 * :3216-3227); num_data_out (device [nblocks], may be NULL): for every block the call has a slot
 * in, the slots of the block filled so far, counted from slot 0: min(k, first_slot + entries - b
 * k).  These are the arrays nfec_tx_list and nfec_encode (batch.num_data) take.  stats (device
 * [2], may be NULL; the caller zeroes it): the packed and rejected counts are added. */
int nfec_stream_pack(const nfec_codec* codec, const nfec_stream_segments* segments, uint32_t segment_size,
                     uint64_t first_slot, uint32_t write_offset, uint32_t flags,
                     const nfec_block_batch* batch, uint16_t* num_data_out, uint16_t* seg_length_out,
                     uint32_t length_stride, uint32_t* stats, void* stream);

/* nfec_stream_unpack (receiver): source slot (b, s), s < k, is selected by nfec_object_write's
 * rule (received NULL, or its bit set in received[b], or status given and status[b] > 0), within
 * the block's nd_b = batch->num_data ? num_data[b] : k source slots: a slot at or past nd_b (a
 * block the sender closed early, nfec_stream_pack's num_data_out) is never selected.  A slot's
 * header is read with one aligned 8-byte load.  Length 0 is a control segment (stream end, or a
 * slot never written: ReadPrivate :3700-3860 treats it so): counted, nothing copied.  With d =
 * (payload_offset - base_offset) mod 2^32 the segment is invalid -- counted, nothing copied --
 * when payload_len > segment_size (ReadPrivate's own test) or d + payload_len > window_bytes.
 * Otherwise slot bytes [8, 8 + len) go to window[d, d + len), window (device memory, window_bytes
 * of it) at any byte alignment.  No other byte of the window is written, or read and written
 * back; the header is network data, and no header value makes the call write outside the window
 * or read outside the slot's own seg_stride bytes.  Per-slot outputs, device [nblocks][out_stride],
 * each may be NULL: offset_out the raw payload_offset, len_out payload_len (0xFFFF for a slot that
 * was not selected; the other two are then not written), msg_start_out payload_msg_start: with
 * them the host runs ReadPrivate's logic (contiguous prefix, message seek by msg_start - 1, stream
 * end) on a few bytes per segment.  stats (device [4], may be NULL; the caller zeroes it):
 * delivered, not selected, control and invalid counts are added. */
int nfec_stream_unpack(const nfec_codec* codec, const nfec_block_batch* batch, const uint32_t* received,
                       uint32_t mask_stride, const int32_t* status, void* window, uint64_t window_bytes,
                       uint32_t base_offset, uint32_t segment_size, uint32_t* offset_out,
                       uint16_t* len_out, uint16_t* msg_start_out, uint32_t out_stride, uint32_t* stats,
                       void* stream);

/* ---- host-resident batched path: same layouts, host pointers (pageable or pinned).
 * Staged through pinned buffers with H2D / compute / D2H overlapped on streams.
 * Synchronous: returns when all outputs are back in host memory.  A codec owns one staging
 * pipeline: host-batch calls (these and the *_host_vectors calls) on one codec from several
 * host threads are serialised; calls on different codecs run concurrently. */
int nfec_encode_host(nfec_codec* codec, const nfec_block_batch* host_batch);
int nfec_decode_host(nfec_codec* codec, const nfec_block_batch* host_batch,
                     const uint16_t* erasure_locs, uint32_t erasure_stride,
                     const uint16_t* erasure_counts, int32_t* status);

/* ---- host segment lists: many blocks, each a list of scattered segment pointers ----
 * The batch form of NormObject::CalculateBlockParity (src/common/normObject.cpp:2203-2229)
 * and of the receiver's NormSenderNode::Decode site (normObject.cpp:1548-1644), where a
 * block is block->SegmentList(): pointers into NORM's segment pool (normSegment.cpp:14-86).
 * vectors[b*(k+m) + s] is block b's slot s: slots [0, numData_b) source, [numData_b,
 * numData_b + m) parity; each holds >= vector_size bytes.  num_data: host [nblocks] or NULL
 * (= k).  Encode writes the parity vectors (XOR into them with NFEC_ACCUMULATE).  Decode
 * writes only the erased source vectors listed in erasure_locs[b*erasure_stride ..] (sorted,
 * erasure_counts[b] entries); parity pointers may be NULL (absent, never dereferenced;
 * MDP reads them as zero).  status (host [nblocks], may be NULL) as nfec_decode.  RS16 never
 * writes an odd last byte.  Synchronous; segments are gathered into pinned staging by host
 * threads, with H2D / compute / D2H overlapped. */
int nfec_encode_host_vectors(nfec_codec* codec, void* const* vectors, uint32_t nblocks,
                             const uint16_t* num_data, uint32_t flags);
int nfec_decode_host_vectors(nfec_codec* codec, void* const* vectors, uint32_t nblocks,
                             const uint16_t* num_data, const uint16_t* erasure_locs,
                             uint32_t erasure_stride, const uint16_t* erasure_counts,
                             int32_t* status, uint32_t flags);

/* ---- asynchronous segment-list batches: receiver-side cross-block batching ----
 * The receiver's decode site (NormObject::HandleObjectMessage -> NormSenderNode::Decode,
 * normObject.cpp:1548-1644, normNode.h:484-487) runs one block per call on NORM's protocol
 * thread.  These queue a batch of blocks on the codec and return at once; the protocol thread
 * keeps receiving and later collects the completion.  Arguments as the synchronous calls; the
 * pointer table, num_data, erasure lists and counts are copied at submission, the segment
 * buffers and the status array must stay valid until the request completes.  A codec runs its
 * requests in submission order on a worker thread of its own; different codecs (one decoder
 * per remote sender, normNode.h:649) run concurrently.  Destroying a codec completes its
 * queued requests first (their handles must still be waited on or were already). */
typedef struct nfec_request nfec_request;
int nfec_encode_host_vectors_async(nfec_codec* codec, void* const* vectors, uint32_t nblocks,
                                   const uint16_t* num_data, uint32_t flags, nfec_request** request);
int nfec_decode_host_vectors_async(nfec_codec* codec, void* const* vectors, uint32_t nblocks,
                                   const uint16_t* num_data, const uint16_t* erasure_locs,
                                   uint32_t erasure_stride, const uint16_t* erasure_counts,
                                   int32_t* status, uint32_t flags, nfec_request** request);
/* 1 when the request has completed, 0 while pending (non-blocking poll). */
int nfec_request_test(nfec_request* request);
/* Blocks until completion, frees the request and returns the call's status code. */
int nfec_request_wait(nfec_request* request);

/* ---- per-call NORM semantics with scattered host vectors (drop-in classes) ---- */
/* NormEncoder::Encode: parity_vectors[i] ^= G[k+i][segment_id] * data over vector_size
 * bytes (RS16: vector_size/2 symbols).  MDP: one in-order LFSR step. Synchronous. */
int nfec_encode_segment(nfec_codec* codec, uint32_t segment_id, const void* data,
                        void* const* parity_vectors);
/* NormDecoder::Decode: returns erasure_count on success, 0 when undecodable, <0 on error. */
int nfec_decode_vectors(nfec_codec* codec, void* const* vector_list, uint32_t num_data,
                        uint32_t erasure_count, const uint32_t* erasure_locs);
/* ---- host CPU per-call paths (NORM's incremental sender, one-block repair) ----
 * NormObject::NextSenderMsg calls Encode once per source segment and reads the parity without
 * a call that ends the block (normObject.cpp:2038-2052), so each call must finish on return:
 * m products of one segment, microseconds of CPU work against ~80 us for a GPU round trip
 * (INTEGRATION.md section 1).  These run on the calling CPU thread: GF(2^8) products by GFNI
 * affine transforms, AVX2 nibble tables or a scalar product table, whichever the CPU has. */
enum { NFEC_HOST_GF_SCALAR = 0, NFEC_HOST_GF_AVX2 = 1, NFEC_HOST_GF_GFNI = 2 };
/* dst[0..bytes) ^= c * src[0..bytes) in the RS8 field (0x11d).  isa: an NFEC_HOST_GF_* form, or
 * < 0 for the best this CPU has.  Returns the form used, NFEC_ENOTSUP when the CPU lacks it. */
int nfec_gf8_addmul_host(void* dst, const void* src, uint8_t c, size_t bytes, int isa);
/* ... over `symbols` native-endian 16-bit symbols in the RS16 field (0x1100B); forms: GFNI or
 * scalar (an AVX2 request runs the scalar form, which is what it returns). */
int nfec_gf16_addmul_host(void* dst, const void* src, uint16_t c, size_t symbols, int isa);
/* Row dot product, the body of nfec_decode_vectors_host:
 *   dst[0..n) = (accumulate ? dst : 0) + sum_j coef[j] * src[j][0..n)
 * over n bytes (bits = 8, RS8 / MDP field) or n native-endian symbols (bits = 16, RS16 field),
 * one pass over dst.  Returns the form used (as above), NFEC_EINVAL / NFEC_ENOTSUP otherwise. */
int nfec_gf_dot_host(int bits, void* dst, const void* const* src, const uint16_t* coef, uint32_t ncols,
                     size_t n, int accumulate, int isa);
/* NormEncoderRS8::Encode (normEncoderRS8.cpp:473-483) on the host: parity_vectors[i] ^=
 * G[k+i][segment_id] * data over vector_size bytes.  RS16 (NormEncoderRS16::Encode,
 * normEncoderRS16.cpp:472-482): the same over vector_size / 2 native-endian symbols, an odd last
 * byte untouched.  MDP (NormEncoderMDP::Encode, normEncoderMDP.cpp:178-211): one LFSR step,
 * s = data ^ parity[0], parity[i] = parity[i+1] ^ g[m-1-i] * s, parity[m-1] = g[0] * s --
 * segments in order, as the reference requires (segment_id is ignored, as there).  Reads only
 * the codec's generator: concurrent calls on one codec are safe (on different blocks). */
int nfec_encode_segment_host(nfec_codec* codec, uint32_t segment_id, const void* data,
                             void* const* parity_vectors);

/* NormDecoderRS8::Decode / NormDecoderRS16::Decode (normEncoderRS8.cpp:652-757, RS16 :650-755)
 * and NormDecoderMDP::Decode (normEncoderMDP.cpp:333-430) on the host CPU, same contract as
 * nfec_decode_vectors.  RS: the block's closed-form repair map (the first surviving parities
 * substitute for the erased source, rs8_plan_rt_kernel's algebra) applied with the GFNI / AVX2
 * region products, XORed into the erased source buffers.  MDP: the closed-form Forney map
 * (mdp_plan_kernel's) over the surviving slots, written over the erased source.  Returns
 * erasure_count, 0 when undecodable or the list is not sorted / in range (block untouched),
 * NFEC_ENOTSUP for RS16 codes past the closed form (min(k, m) > 64).  A one-block repair of a
 * NORM-sized block is tens of microseconds of CPU work, below the GPU round trip. */
int nfec_decode_vectors_host(nfec_codec* codec, void* const* vectors, uint32_t num_data,
                             uint32_t erasure_count, const uint32_t* erasure_locs);
/* 1 when nfec_decode_vectors_host is the faster path for this call, else 0 (the drop-in
 * Decode's choice), from the measured latencies: RS8 while erasures x numData x vector bytes
 * stays within 256 MiB, MDP while erasures x (numData + numParity) x vector bytes stays within
 * 512 MiB, RS16 (min(k, m) <= 64) while erasures x numData x symbols stays within 64 Mi. */
int nfec_decode_host_preferred(const nfec_codec* codec, uint32_t num_data, uint32_t erasure_count);

/* sizeof() of the drop-in class NormEncoder<kind> (decoder = 0) or NormDecoder<kind>
 * (decoder = 1) as the library was compiled (include/norm_fec/normEncoder*.h), 0 for an
 * unknown kind: a NORM build can check that its translation units see the same layout. */
size_t nfec_dropin_sizeof(int kind, int decoder);

/* The host worker pool every host-batch copy of 4 MiB or more runs on (one per process): its
 * workers (the cores the job may use -- the affinity mask capped by the cgroup cpu.max quota --
 * or NFEC_HOST_THREADS, at most 64), the usable and the visible cores.  All stripes of all codecs
 * share it; smaller copies run on the calling thread. */
int nfec_host_threads(uint32_t* pool, uint32_t* usable_cores, uint32_t* visible_cores);
/* Self-check of that pool (tests): runs `pieces` pieces on it.  mode 0: every piece counts once;
 * 1: piece 1 throws std::bad_alloc; 2: piece 1 throws std::runtime_error.  Returns the pieces that
 * ran to completion (mode 0: all of them), or the pool's error status (NFEC_ENOMEM / NFEC_EINVAL)
 * once every piece has run -- a throwing piece neither ends the process nor leaves the call
 * waiting.  Safe in a child forked after the pool started (its pieces then run inline). */
int nfec_util_pool_check(uint32_t pieces, int mode);
/* Host-side rate probe of the segment-list gather (no GPU): nstripes driver threads, one per
 * would-be device, each gather their contiguous block range [i*B/N, (i+1)*B/N) of the pointer
 * table vectors[b*slots + s] (slots vectors of vector_size bytes per block) into staging of their
 * own in the pipelines' 128 MiB chunks, through the same pool as nfec_*_host_vectors.  *seconds:
 * the mean wall time of one pass over all blocks; *max_active (may be NULL): the most copy
 * pieces that ran at once during the probe (at most the pool's size). */
int nfec_util_gather_probe(void* const* vectors, uint32_t nblocks, uint32_t slots, uint32_t vector_size,
                           uint32_t nstripes, uint32_t reps, double* seconds, uint32_t* max_active);
/* ---- synthetic workload utilities (device kernels; SURVEY.md 8d definitions) ----
 * fill: source slots [0, numData) of every block with the splitmix64 stream
 *       word w of (block b, slot s) = mix(seed ^ ((b0+b)<<20) ^ s + (w+1)*0x9E3779B97F4A7C15).
 * erasures: per block `count` sorted distinct indices in [0, range), Fisher-Yates over the
 *           counter stream mix(seed ^ 0xE7A5E7A500000000 ^ (b0+b) + (i+1)*gamma).
 * zero: zero the listed slots of every block (the receiver's zero-fill, normObject.cpp:1579).
 * stream_copy: device-to-device copy of `bytes` (16-byte aligned pointers and size) by a
 *       streaming kernel, for the bench's achievable-HBM-rate figure. */
int nfec_util_fill(const nfec_block_batch* batch, uint32_t num_data, uint32_t vector_size,
                   uint64_t seed, uint64_t first_block, void* stream);
int nfec_util_erasures(uint16_t* erasure_locs, uint32_t erasure_stride, uint16_t* erasure_counts,
                       uint32_t nblocks, uint32_t range, uint32_t count, uint64_t seed,
                       uint64_t first_block, void* stream);
int nfec_util_zero_slots(const nfec_block_batch* batch, const uint16_t* erasure_locs,
                         uint32_t erasure_stride, const uint16_t* erasure_counts,
                         uint32_t vector_size, void* stream);
int nfec_util_stream_copy(void* dst, const void* src, uint64_t bytes, void* stream);

/* ---- NORM wire format on the FEC path (host only; no device work) ----
 * The FEC Object Transmission Information header extension (type 64) a sender attaches to
 * NORM_INFO/NORM_DATA and a receiver reads to build its decoder, the FEC payload ID in every
 * NORM_DATA, and the codec choice each side makes from them.  Big-endian on the wire. */
typedef struct nfec_fti {
    uint8_t fec_id;         /* 2, 5 or 129 */
    uint8_t fec_m;          /* field bits: 8 or 16 for fec_id 2; 8 for 5 and 129 (read side) */
    uint8_t fec_group_size; /* fec_id 2 'G' (symbols per packet); read as 1 for 5, 129 */
    uint8_t reserved;
    uint16_t instance_id;   /* fec_id 129 */
    uint16_t segment_size;
    uint16_t num_data;      /* FEC max block length (u8 on the wire for fec_id 5) */
    uint16_t num_parity;
    uint64_t object_size;   /* NormObjectSize, 48 bits */
} nfec_fti;

/* NormFtiExtension2/5/129::SetObjectSize...SetFecNumParity (normMessage.h:785-1029):
 * writes the whole extension (16 bytes; 12 for fec_id 5) into ext and returns its length,
 * NFEC_EINVAL for an unknown fec_id, cap too small or object_size >= 2^48, NFEC_ERANGE when
 * num_data/num_parity do not fit fec_id 5's u8 fields. */
int nfec_fti_write(const nfec_fti* fti, void* ext, size_t cap);
/* The matching getters: parses ext (len bytes) for fec_id; returns bytes consumed or
 * NFEC_EINVAL (unknown fec_id, short buffer, type != 64 or length field too small). */
int nfec_fti_read(uint8_t fec_id, const void* ext, size_t len, nfec_fti* out);
/* NormPayloadId (normMessage.h:396-567): 4 bytes for fec_id 2 and 5, 8 for 129, 0 unknown. */
int nfec_payload_id_length(uint8_t fec_id);
/* fec 2/m 8 and fec 5: u32 block<<8 | symbol; fec 2/m 16: u16 block, u16 symbol; fec 129:
 * u32 block, u16 block length, u16 symbol.  Return the length, or NFEC_EINVAL.
 * block_len is only carried by fec 129 (read returns 0 for it otherwise; may be NULL). */
int nfec_payload_id_write(uint8_t fec_id, uint8_t fec_m, uint32_t block_id, uint16_t symbol_id,
                          uint16_t block_len, void* out);
int nfec_payload_id_read(uint8_t fec_id, uint8_t fec_m, const void* in, uint32_t* block_id,
                         uint16_t* symbol_id, uint16_t* block_len);
/* Sender choice (NormSession::StartSender, normSession.cpp:764-898): numParity == 0 -> no
 * codec (*kind = 0), fec_id_pref (0 = 5), m 8; numData + numParity <= 255 -> RS8 with
 * fec_id_pref (0 = 5) and m 8, or MDP/129 when assume_mdp; else RS16, fec 2, m 16. */
int nfec_sender_codec(uint16_t num_data, uint16_t num_parity, uint8_t fec_id_pref, int assume_mdp,
                      int* kind, uint8_t* fec_id, uint8_t* fec_m);
/* Receiver choice (NormSenderNode::AllocateBuffers, normNode.cpp:290-356): fec 2 m 8 -> RS8,
 * m 16 -> RS16; fec 5 -> RS8; fec 129 -> MDP when assume_mdp, RS8 for instance 0; anything
 * else NFEC_ENOTSUP. */
int nfec_receiver_codec(uint8_t fec_id, uint8_t fec_m, uint16_t instance_id, int assume_mdp,
                        int* kind);
/* The codec vector size for a segment size: segment_size + the 8-byte stream payload header
 * NORM codes along with the data (NormDataMsg::GetStreamPayloadHeaderLength). */
uint32_t nfec_vector_size(uint16_t segment_size);

/* ---- npc: the offline file precoder (src/common/normPrecode.cpp) on the GPU path ----
 * .npc files are byte-identical to the reference tool's for the same input and parameters
 * (meta segment, CRC-32 per segment, interleaving, the encoder's segment-id rotation). */
typedef struct nfec_npc_params {
    uint32_t segment_size;   /* "segment": 12..8192 bytes, the last 4 hold the segment's CRC-32 */
    uint32_t num_data;       /* "block": used when parity_fraction < 0 */
    uint32_t num_parity;     /* "parity" */
    double parity_fraction;  /* "auto" percent / 100; >= 0 sizes the block from the file size.
                                The reference's default is 100.0 (auto mode, 100x parity). */
    uint64_t b_max;          /* "bmax": auto-mode block cap */
    uint64_t i_max;          /* "imax": interleaver max dimension, 0 = none */
} nfec_npc_params;

typedef struct nfec_npc_layout {
    uint64_t num_segments;    /* segments in the .npc file */
    uint64_t input_segments;  /* meta + data segments */
    uint64_t num_blocks;
    uint32_t num_data, num_parity;
    uint32_t last_block_data;     /* numData of the last FEC block */
    uint32_t segment_size;
    uint32_t last_segment_bytes;  /* encode: file bytes in the last data segment (0 on decode) */
    int32_t kind;                 /* NFEC_RS8, or NFEC_RS16 when numData + numParity > 256 */
    uint64_t il_width, il_height, il_size, i_max;
} nfec_npc_layout;

/* NormPrecodeApp's constructor defaults (normPrecode.cpp:111-115). */
void nfec_npc_default_params(nfec_npc_params* params);
/* Block sizing (OnStartup :383-434) and file layout (Encode :611-637 / Decode :886-909,
 * InitInterleaver :450-462) for an input of file_size bytes.  Host only. */
int nfec_npc_layout_for(const nfec_npc_params* params, uint64_t file_size, int encode,
                        nfec_npc_layout* out);
/* File slot of FEC-order segments [first, first+count) (ComputeInterleaverOffset :465-556
 * divided by segment_size).  Host only.  NFEC_ENOTSUP where the reference's remap fails. */
int nfec_npc_positions(const nfec_npc_layout* layout, uint64_t first, uint64_t count, uint64_t* pos);
/* NormPrecodeApp::Encode: in_path -> out_path (.npc) on HIP device `device`. */
int nfec_npc_encode_file(int device, const char* in_path, const char* out_path,
                         const nfec_npc_params* params);
/* NormPrecodeApp::Decode: out_path NULL writes to the file name stored in the meta segment
 * (current directory), as the reference does; that name goes to name_out when given.
 * NFEC_ERANGE when a block has more bad segments than parity (the reference's fatal case). */
int nfec_npc_decode_file(int device, const char* in_path, const char* out_path,
                         const nfec_npc_params* params, uint64_t* out_bytes, char* name_out,
                         size_t name_cap);
/* The same file passes over several GPUs (devices[0..num_devices), may repeat a device):
 * device i takes the i-th contiguous range of FEC blocks, with its own codec, staging and host
 * thread; host copy threads (NFEC_NPC_THREADS) are shared among them.  Output bytes are
 * identical to the one-device call.  NFEC_EINVAL for an empty list or a device index out of
 * range.  The one-device functions above are these with a list of one. */
int nfec_npc_encode_file_multi(const int32_t* devices, int32_t num_devices, const char* in_path,
                               const char* out_path, const nfec_npc_params* params);
int nfec_npc_decode_file_multi(const int32_t* devices, int32_t num_devices, const char* in_path,
                               const char* out_path, const nfec_npc_params* params,
                               uint64_t* out_bytes, char* name_out, size_t name_cap);
/* CRC-32 (npc's ComputeCRC32, :1303-1313) of the first len bytes of slots [0, slots) of every
 * block of a device batch -> crc[b*slots + s] (device), asynchronously on stream. */
int nfec_crc32_slots(const nfec_block_batch* batch, uint32_t slots, uint32_t len, uint32_t* crc,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NFEC_H */
