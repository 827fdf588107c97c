"""ctypes binding of libnfec.so (include/nfec.h).

The library is built in-tree (norm_amd/_lib/libnfec.so, see norm_amd/Makefile and
__graft_entry__.build()).  There is no fallback: if the library is missing or a call
fails, an exception is raised.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# NFEC_LIBRARY selects another build of the same ABI: the diagnostic library with the A/B
# variants and probes of the kernels (make -C norm_amd diag -> _lib/libnfec_diag.so)
PRODUCT_LIB_PATH = os.path.join(_HERE, "_lib", "libnfec.so")
LIB_PATH = os.environ.get("NFEC_LIBRARY") or PRODUCT_LIB_PATH
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nfec.h")

NFEC_RS8, NFEC_RS16, NFEC_MDP = 1, 2, 3
NFEC_OK, NFEC_EINVAL, NFEC_ENOMEM, NFEC_EDEVICE, NFEC_ERANGE, NFEC_ENOTSUP = 0, -1, -2, -3, -4, -5
NFEC_ACCUMULATE = 1
NFEC_STREAM_EOM, NFEC_STREAM_FLUSH = 1, 2
NFEC_STREAM_END = 1
NFEC_NACK_INFO = 1
# nfec_rx_repair_requests: a block's class, a request's form and flags
NACK_SILENT, NACK_NEEDING, NACK_ABSENT = 0, 1, 2
REPAIR_ITEMS, REPAIR_RANGES = 1, 2
REPAIR_SEGMENT, REPAIR_BLOCK, REPAIR_INFO, REPAIR_OBJECT = 1, 2, 4, 8
# nfec_tx_repair_state: the object word
NFEC_TX_REPAIR_OBJECT, NFEC_TX_REPAIR_INFO, NFEC_TX_PENDING_INFO = 1, 2, 4
# nfec_rx_repair_state: the object word
NFEC_RX_REPAIR_OBJECT, NFEC_RX_REPAIR_INFO = 1, 2
# nfec_rx_ingest_data / nfec_rx_parse_data_host: a datagram's class
(NFEC_DGRAM_UNREADABLE, NFEC_DGRAM_OTHER_TYPE, NFEC_DGRAM_MALFORMED, NFEC_DGRAM_OTHER_SENDER, NFEC_DGRAM_OTHER_CODE,
 NFEC_DGRAM_OTHER_OBJECT, NFEC_DGRAM_REJECTED, NFEC_DGRAM_DUPLICATE, NFEC_DGRAM_PLACED) = range(9)
NFEC_DGRAM_CLASSES = NFEC_DGRAM_PARSED = 9
# nfec_rx_ingest_control / nfec_ctl_parse_host: a control datagram's class, the filter's flags
(NFEC_CTL_UNREADABLE, NFEC_CTL_OTHER_TYPE, NFEC_CTL_MALFORMED, NFEC_CTL_OTHER_FLAVOR, NFEC_CTL_OWN, NFEC_CTL_OTHER_SENDER,
 NFEC_CTL_OTHER_INSTANCE, NFEC_CTL_NACK, NFEC_CTL_REPAIR_ADV) = range(9)
NFEC_CTL_CLASSES = 9
NFEC_CTL_EXTENDED = 0x80
NFEC_CTL_ANY_INSTANCE, NFEC_CTL_TAKE_NACK, NFEC_CTL_TAKE_ADV = 1, 2, 4
NFEC_FEATURE_RS16_TOEPLITZ, NFEC_FEATURE_RS16_TOEPLITZ2 = 1, 2
NFEC_OPT_RS16_SHARED_TABLES, NFEC_OPT_RS16_TOEPLITZ_OFF, NFEC_OPT_RS16_TOEPLITZ_ON, NFEC_OPT_HOST_ONLY = 1, 2, 4, 8
NFEC_OPT_RS16_TOEPLITZ_ONE_LEVEL = 16
# encode paths (nfec_codec_encode_paths)
NFEC_PATH_FIXED, NFEC_PATH_RUNTIME, NFEC_PATH_RS16_SPLIT, NFEC_PATH_RS16_PRODUCT, NFEC_PATH_GENERIC = 0, 1, 2, 3, 4
NFEC_PATH_COUNT = 5
PATH_NAMES = ("fixed", "runtime", "rs16_split", "rs16_product", "generic")
NFEC_DPATH_COUNT = 4
DPATH_NAMES = ("fixed", "runtime", "rs16_tower", "generic")
NFEC_HOST_GF_SCALAR, NFEC_HOST_GF_AVX2, NFEC_HOST_GF_GFNI = 0, 1, 2


class NfecError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed with {code}: {last_error()}")
        self.code = code


class BlockBatch(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_void_p),
        ("block_stride", ctypes.c_uint64),
        ("seg_stride", ctypes.c_uint32),
        ("nblocks", ctypes.c_uint32),
        ("num_data", ctypes.c_void_p),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class RxSegments(ctypes.Structure):
    """nfec_rx_segments: received segments in arrival order (device arrays)."""
    _fields_ = [
        ("payloads", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("block_index", ctypes.c_void_p),
        ("symbol_id", ctypes.c_void_p),
        ("length", ctypes.c_void_p),
        ("count", ctypes.c_uint32),
    ]


class RxMessages(ctypes.Structure):
    """nfec_rx_messages: the wire buffer and where each message's payload lies (device arrays)."""
    _fields_ = [
        ("payloads", ctypes.c_void_p),
        ("payload_bytes", ctypes.c_uint64),
        ("offsets", ctypes.c_void_p),
        ("length", ctypes.c_void_p),
        ("count", ctypes.c_uint32),
        ("count_dev", ctypes.c_void_p),
    ]


class TxRepairStateStruct(ctypes.Structure):
    """nfec_tx_repair_state: the sender's repair state (device arrays, or host arrays for the *_host entries)."""
    _fields_ = [
        ("repair", ctypes.c_void_p),
        ("parity", ctypes.c_void_p),
        ("block_repair", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
    ]


class RxRepairStateStruct(ctypes.Structure):
    """nfec_rx_repair_state: a receiver's suppression state (device arrays, or host arrays for the *_host entries)."""
    _fields_ = [
        ("repair", ctypes.c_void_p),
        ("block_repair", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
    ]


class TxSegments(ctypes.Structure):
    """nfec_tx_segments: the wire buffer and the transmission list (device arrays)."""
    _fields_ = [
        ("payloads", ctypes.c_void_p),
        ("payload_bytes", ctypes.c_uint64),
        ("offsets", ctypes.c_void_p),
        ("block_index", ctypes.c_void_p),
        ("symbol_id", ctypes.c_void_p),
        ("length", ctypes.c_void_p),
        ("count", ctypes.c_uint32),
        ("count_dev", ctypes.c_void_p),
    ]


class DataHeader(ctypes.Structure):
    """nfec_data_header: the NORM_DATA header fields the messages of one call share."""
    _fields_ = [
        ("source_id", ctypes.c_uint32),
        ("instance_id", ctypes.c_uint16),
        ("first_sequence", ctypes.c_uint16),
        ("grtt", ctypes.c_uint8),
        ("backoff", ctypes.c_uint8),
        ("gsize", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("fec_id", ctypes.c_uint8),
        ("fec_m", ctypes.c_uint8),
        ("object_id", ctypes.c_uint16),
        ("ext", ctypes.c_uint8 * 16),
        ("ext_bytes", ctypes.c_uint8),
    ]


class DataFilter(ctypes.Structure):
    """nfec_data_filter: the sender, code and object one receiver call takes."""
    _fields_ = [
        ("source_id", ctypes.c_uint32),
        ("instance_id", ctypes.c_uint16),
        ("fec_id", ctypes.c_uint8),
        ("fec_m", ctypes.c_uint8),
        ("object_id", ctypes.c_uint16),
    ]


class NackHeader(ctypes.Structure):
    """nfec_nack_header: the NORM_NACK header fields the messages of one call share."""
    _fields_ = [
        ("source_id", ctypes.c_uint32),
        ("sender_id", ctypes.c_uint32),
        ("instance_id", ctypes.c_uint16),
        ("first_sequence", ctypes.c_uint16),
        ("sequence_step", ctypes.c_uint16),
        ("grtt_response_sec", ctypes.c_uint32),
        ("grtt_response_usec", ctypes.c_uint32),
        ("ext", ctypes.c_uint8 * 12),
        ("ext_bytes", ctypes.c_uint8),
    ]


class AdvHeader(ctypes.Structure):
    """nfec_adv_header: the header of one NORM_CMD(REPAIR_ADV)."""
    _fields_ = [
        ("source_id", ctypes.c_uint32),
        ("instance_id", ctypes.c_uint16),
        ("sequence", ctypes.c_uint16),
        ("grtt", ctypes.c_uint8),
        ("backoff", ctypes.c_uint8),
        ("gsize", ctypes.c_uint8),
        ("ext", ctypes.c_uint8 * 12),
        ("ext_bytes", ctypes.c_uint8),
    ]


class CtlFilter(ctypes.Structure):
    """nfec_ctl_filter: whose control messages one intake call takes."""
    _fields_ = [
        ("sender_id", ctypes.c_uint32),
        ("instance_id", ctypes.c_uint16),
        ("local_id", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class ObjectLayout(ctypes.Structure):
    """nfec_object_layout: the FEC block partition of a NORM data object."""
    _fields_ = [
        ("object_size", ctypes.c_uint64),
        ("segment_size", ctypes.c_uint32),
        ("num_data", ctypes.c_uint32),
        ("num_segments", ctypes.c_uint64),
        ("num_blocks", ctypes.c_uint32),
        ("large_block_size", ctypes.c_uint32),
        ("large_block_count", ctypes.c_uint32),
        ("small_block_size", ctypes.c_uint32),
        ("small_block_count", ctypes.c_uint32),
        ("final_block_id", ctypes.c_uint32),
        ("final_segment_size", ctypes.c_uint32),
    ]


class StreamState(ctypes.Structure):
    """nfec_stream_state: what framing a stream's writes carries from one call to the next."""
    _fields_ = [
        ("write_offset", ctypes.c_uint32),
        ("msg_start_pending", ctypes.c_uint32),
        ("carry_bytes", ctypes.c_uint32),
        ("carry_msg_start", ctypes.c_uint32),
        ("next_slot", ctypes.c_uint64),
    ]


class StreamSegments(ctypes.Structure):
    """nfec_stream_segments: the stream bytes and the segment table (device arrays)."""
    _fields_ = [
        ("bytes", ctypes.c_void_p),
        ("stream_bytes", ctypes.c_uint64),
        ("seg_start", ctypes.c_void_p),
        ("seg_len", ctypes.c_void_p),
        ("seg_msg_start", ctypes.c_void_p),
        ("count", ctypes.c_uint32),
        ("count_dev", ctypes.c_void_p),
    ]


class CodecInfo(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("num_data", ctypes.c_uint32),
        ("num_parity", ctypes.c_uint32),
        ("vector_size", ctypes.c_uint32),
        ("symbol_bytes", ctypes.c_uint32),
    ]


class CodecConfig(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("num_data", ctypes.c_uint32),
        ("num_parity", ctypes.c_uint32),
        ("vector_size", ctypes.c_uint32),
        ("devices", ctypes.POINTER(ctypes.c_int32)),
        ("num_devices", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class Fti(ctypes.Structure):
    _fields_ = [
        ("fec_id", ctypes.c_uint8),
        ("fec_m", ctypes.c_uint8),
        ("fec_group_size", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("instance_id", ctypes.c_uint16),
        ("segment_size", ctypes.c_uint16),
        ("num_data", ctypes.c_uint16),
        ("num_parity", ctypes.c_uint16),
        ("object_size", ctypes.c_uint64),
    ]


class NpcParams(ctypes.Structure):
    _fields_ = [
        ("segment_size", ctypes.c_uint32),
        ("num_data", ctypes.c_uint32),
        ("num_parity", ctypes.c_uint32),
        ("parity_fraction", ctypes.c_double),
        ("b_max", ctypes.c_uint64),
        ("i_max", ctypes.c_uint64),
    ]


class NpcLayout(ctypes.Structure):
    _fields_ = [
        ("num_segments", ctypes.c_uint64),
        ("input_segments", ctypes.c_uint64),
        ("num_blocks", ctypes.c_uint64),
        ("num_data", ctypes.c_uint32),
        ("num_parity", ctypes.c_uint32),
        ("last_block_data", ctypes.c_uint32),
        ("segment_size", ctypes.c_uint32),
        ("last_segment_bytes", ctypes.c_uint32),
        ("kind", ctypes.c_int32),
        ("il_width", ctypes.c_uint64),
        ("il_height", ctypes.c_uint64),
        ("il_size", ctypes.c_uint64),
        ("i_max", ctypes.c_uint64),
    ]


_P = ctypes.c_void_p
_U8 = ctypes.c_uint8
_U16 = ctypes.c_uint16
_U32 = ctypes.c_uint32
_U64 = ctypes.c_uint64
_I = ctypes.c_int
_SIGS = {
    "nfec_abi_version": (_I, []),
    "nfec_build_id": (ctypes.c_char_p, []),
    "nfec_device_count": (_I, []),
    "nfec_last_error": (ctypes.c_char_p, []),
    "nfec_build_generator": (_I, [_I, _U32, _U32, _P, ctypes.c_size_t]),
    "nfec_codec_create": (_I, [_I, _I, _U32, _U32, _U32, ctypes.POINTER(_P)]),
    "nfec_codec_create_ex": (_I, [ctypes.POINTER(CodecConfig), ctypes.POINTER(_P)]),
    "nfec_codec_num_devices": (_I, [_P, ctypes.POINTER(ctypes.c_int32), _U32]),
    "nfec_codec_destroy": (None, [_P]),
    "nfec_codec_get_info": (_I, [_P, ctypes.POINTER(CodecInfo)]),
    "nfec_codec_features": (_I, [_P]),
    "nfec_codec_encode_paths": (_I, [_P, ctypes.POINTER(_U64), _U32]),
    "nfec_codec_decode_paths": (_I, [_P, ctypes.POINTER(_U64), _U32]),
    "nfec_codec_tail_batches": (_I, [_P, ctypes.POINTER(_U64), _U32]),
    "nfec_codec_get_generator": (_I, [_P, _P, ctypes.c_size_t]),
    "nfec_encode": (_I, [_P, ctypes.POINTER(BlockBatch), _P]),
    "nfec_decode": (_I, [_P, ctypes.POINTER(BlockBatch), _P, _U32, _P, _P, _P]),
    "nfec_rx_place": (_I, [_P, ctypes.POINTER(BlockBatch), ctypes.POINTER(RxSegments), _P, _U32, _P, _P]),
    "nfec_rx_ingest": (_I, [_P, ctypes.POINTER(BlockBatch), ctypes.POINTER(RxMessages), _U8, _U8, _U32, _P, _U32, _P, _P,
                            _P, _P]),
    "nfec_rx_parse_host": (_I, [_U8, _U8, _U32, _P, _U64, _P, _P, _U32, _P, _P, _P]),
    "nfec_rx_erasures": (_I, [_P, _P, _U32, _P, _U32, _P, _U32, _P, _P]),
    "nfec_decode_received": (_I, [_P, ctypes.POINTER(BlockBatch), _P, _U32, _P, _P]),
    "nfec_rx_erasures_host": (_I, [_U32, _U32, _P, _U32, _P, _U32, _P, _U32, _P]),
    "nfec_rx_repair_requests": (_I, [_P, _P, _U32, _P, _U32, _U8, _U8, _U16, _U32, _U32, _U32, _P, _U64, _P, _P, _P]),
    "nfec_rx_repair_requests_host": (_I, [_U32, _U32, _P, _U32, _P, _U32, _U8, _U8, _U16, _U32, _U32, _U32, _P, _U64, _P,
                                          _P]),
    "nfec_repair_parse_host": (_I, [_U8, _U8, _P, _U64, _P, _P, _P, _P, _U32, ctypes.POINTER(_U64)]),
    "nfec_nack_scan_combine_host": (None, [_P, _P, _P]),
    "nfec_tx_list": (_I, [_P, _P, _U32, _P, _U32, _P, _U32, _U32, _P, _P, _P, _P, _U32, _P, _P]),
    "nfec_tx_list_host": (_I, [_U32, _U32, _U32, _P, _U32, _P, _U32, _P, _U32, _U32, _P, _P, _P, _P, _U32, _P]),
    "nfec_tx_emit": (_I, [_P, ctypes.POINTER(BlockBatch), ctypes.POINTER(TxSegments), _U8, _U8, _U32, _P, _U32, _P,
                          _P]),
    "nfec_data_header_bytes": (_I, [_U8, _U8]),
    "nfec_tx_emit_data": (_I, [_P, ctypes.POINTER(BlockBatch), ctypes.POINTER(TxSegments), ctypes.POINTER(DataHeader), _U32,
                               _P, _U32, _P, _P, _P, _P]),
    "nfec_rx_ingest_data": (_I, [_P, ctypes.POINTER(BlockBatch), ctypes.POINTER(RxMessages), ctypes.POINTER(DataFilter),
                                 _U32, _P, _U32, _P, _P, _P, _P, _P, _P, _P]),
    "nfec_data_header_write_host": (_I, [ctypes.POINTER(DataHeader), _U32, _U32, _U16, _U16, _P, ctypes.c_size_t]),
    "nfec_rx_parse_data_host": (_I, [ctypes.POINTER(DataFilter), _U32, _P, _U64, _P, _P, _U32, _P, _P, _P, _P, _P, _P, _P,
                                     _P]),
    "nfec_rx_data_chunks_host": (_I, [_U64, _U16, _P]),
    "nfec_nack_header_bytes": (_I, [_U8]),
    "nfec_adv_header_bytes": (_I, [_U8]),
    "nfec_nack_fragment": (_I, [_P, _P, _U64, _P, _P, _U32, _U8, _U32, ctypes.POINTER(NackHeader), _P, _U64, _U32, _P, _P,
                                _U32, _P, _P, _U64, _P]),
    "nfec_nack_fragment_workspace_bytes": (_U64, [_U64, _U32]),
    "nfec_tx_repair_adv_message": (_I, [_P, _P, _U64, _P, _U8, _U32, ctypes.POINTER(AdvHeader), _P, _U64, _P, _P, _P]),
    "nfec_rx_ingest_control": (_I, [_P, ctypes.POINTER(RxMessages), ctypes.POINTER(CtlFilter), _P, _P, _P, _P, _P, _P, _P]),
    "nfec_nack_fragment_host": (_I, [_P, _U64, _U8, _U32, ctypes.POINTER(NackHeader), _P, _U64, _U32, _P, _P, _U32, _P]),
    "nfec_nack_header_write_host": (_I, [ctypes.POINTER(NackHeader), _U32, _P, ctypes.c_size_t]),
    "nfec_adv_message_host": (_I, [_P, _U64, _U8, _U32, ctypes.POINTER(AdvHeader), _P, _U64, _P]),
    "nfec_ctl_parse_host": (_I, [ctypes.POINTER(CtlFilter), _P, _U64, _P, _P, _U32, _P, _P, _P, _P, _P, _P]),
    "nfec_tx_handle_nacks": (_I, [_P, ctypes.POINTER(RxMessages), _U8, _U8, _U16, _U32, _P, _U32, _U32, _U32,
                                  ctypes.POINTER(TxRepairStateStruct), _U32, _P, _U64, _P, _P]),
    "nfec_tx_nack_workspace_bytes": (_U64, [_U32, _U32, _U32]),
    "nfec_tx_handle_nacks_host": (_I, [_U32, _U32, ctypes.POINTER(RxMessages), _U8, _U8, _U16, _U32, _P, _U32, _U32, _U32,
                                       ctypes.POINTER(TxRepairStateStruct), _U32, _P]),
    "nfec_tx_activate_repairs": (_I, [_P, _P, _U32, _U32, _P, _U32, ctypes.POINTER(TxRepairStateStruct), _P, _P]),
    "nfec_tx_activate_repairs_host": (_I, [_U32, _U32, _P, _U32, _U32, _P, _U32, ctypes.POINTER(TxRepairStateStruct), _P]),
    "nfec_tx_end_blocks": (_I, [_P, _P, _U32, _P, _U32, ctypes.POINTER(TxRepairStateStruct), _P]),
    "nfec_tx_end_blocks_host": (_I, [_U32, _U32, _P, _U32, _P, _U32, ctypes.POINTER(TxRepairStateStruct)]),
    "nfec_rx_handle_repair_content": (_I, [_P, ctypes.POINTER(RxMessages), _U8, _U8, _U16, _U32, _P, _U32, _P, _U32,
                                           ctypes.POINTER(RxRepairStateStruct), _P, _P]),
    "nfec_rx_handle_repair_content_host": (_I, [_U32, _U32, ctypes.POINTER(RxMessages), _U8, _U8, _U16, _U32, _P, _U32, _P,
                                                _U32, ctypes.POINTER(RxRepairStateStruct), _P]),
    "nfec_rx_repair_pending": (_I, [_P, _P, _U32, _P, _U32, ctypes.POINTER(RxRepairStateStruct), _U32, _P, _P, _P]),
    "nfec_rx_repair_pending_host": (_I, [_U32, _U32, _P, _U32, _P, _U32, ctypes.POINTER(RxRepairStateStruct), _U32, _P, _P]),
    "nfec_tx_repair_adv": (_I, [_P, ctypes.POINTER(TxRepairStateStruct), _U32, _P, _U32, _U8, _U8, _U16, _U32, _U32, _P,
                                _U64, _P, _P, _P]),
    "nfec_tx_repair_adv_host": (_I, [_U32, _U32, ctypes.POINTER(TxRepairStateStruct), _U32, _P, _U32, _U8, _U8, _U16, _U32,
                                     _U32, _P, _U64, _P, _P]),
    "nfec_object_layout_for": (_I, [_U64, _U32, _U32, ctypes.POINTER(ObjectLayout)]),
    "nfec_object_segment": (_I, [ctypes.POINTER(ObjectLayout), _U32, _U32, ctypes.POINTER(_U64), ctypes.POINTER(_U32)]),
    "nfec_object_block_sizes": (_I, [ctypes.POINTER(ObjectLayout), _U32, _U32, _P]),
    "nfec_object_read": (_I, [_P, ctypes.POINTER(ObjectLayout), _P, _U64, _U32, ctypes.POINTER(BlockBatch), _P, _P, _U32,
                              _P]),
    "nfec_object_write": (_I, [_P, ctypes.POINTER(ObjectLayout), _P, _U64, _U32, ctypes.POINTER(BlockBatch), _P, _U32,
                               _P, _P, _P]),
    "nfec_stream_frame_host": (_I, [_U32, _P, _P, _U32, ctypes.POINTER(StreamState), _P, _P, _P, _U32, _P]),
    "nfec_stream_frame": (_I, [_P, _U32, _P, _P, _U32, StreamState, _P, _P, _P, _P, _U32, _P, _P, _P]),
    "nfec_stream_pack": (_I, [_P, ctypes.POINTER(StreamSegments), _U32, _U64, _U32, _U32, ctypes.POINTER(BlockBatch), _P,
                              _P, _U32, _P, _P]),
    "nfec_stream_unpack": (_I, [_P, ctypes.POINTER(BlockBatch), _P, _U32, _P, _P, _U64, _U32, _U32, _P, _P, _P, _U32, _P,
                                _P]),
    "nfec_encode_host": (_I, [_P, ctypes.POINTER(BlockBatch)]),
    "nfec_decode_host": (_I, [_P, ctypes.POINTER(BlockBatch), _P, _U32, _P, _P]),
    "nfec_encode_host_vectors": (_I, [_P, _P, _U32, _P, _U32]),
    "nfec_decode_host_vectors": (_I, [_P, _P, _U32, _P, _P, _U32, _P, _P, _U32]),
    "nfec_encode_host_vectors_async": (_I, [_P, _P, _U32, _P, _U32, _P]),
    "nfec_decode_host_vectors_async": (_I, [_P, _P, _U32, _P, _P, _U32, _P, _P, _U32, _P]),
    "nfec_request_test": (_I, [_P]),
    "nfec_request_wait": (_I, [_P]),
    "nfec_encode_segment": (_I, [_P, _U32, _P, _P]),
    "nfec_encode_segment_host": (_I, [_P, _U32, _P, _P]),
    "nfec_gf8_addmul_host": (_I, [_P, _P, _U8, ctypes.c_size_t, _I]),
    "nfec_gf16_addmul_host": (_I, [_P, _P, ctypes.c_uint16, ctypes.c_size_t, _I]),
    "nfec_gf_dot_host": (_I, [_I, _P, _P, _P, ctypes.c_uint32, ctypes.c_size_t, _I, _I]),
    "nfec_decode_vectors_host": (_I, [_P, _P, _U32, _U32, _P]),
    "nfec_decode_host_preferred": (_I, [_P, _U32, _U32]),
    "nfec_decode_vectors": (_I, [_P, _P, _U32, _U32, _P]),
    "nfec_dropin_sizeof": (ctypes.c_size_t, [_I, _I]),
    "nfec_util_fill": (_I, [ctypes.POINTER(BlockBatch), _U32, _U32, _U64, _U64, _P]),
    "nfec_util_erasures": (_I, [_P, _U32, _P, _U32, _U32, _U32, _U64, _U64, _P]),
    "nfec_util_zero_slots": (_I, [ctypes.POINTER(BlockBatch), _P, _U32, _P, _U32, _P]),
    "nfec_util_stream_copy": (_I, [_P, _P, _U64, _P]),
    "nfec_host_threads": (_I, [ctypes.POINTER(_U32), ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    "nfec_util_pool_check": (_I, [_U32, _I]),
    "nfec_util_gather_probe": (_I, [_P, _U32, _U32, _U32, _U32, _U32, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(_U32)]),
    "nfec_fti_write": (_I, [ctypes.POINTER(Fti), _P, ctypes.c_size_t]),
    "nfec_fti_read": (_I, [_U8, _P, ctypes.c_size_t, ctypes.POINTER(Fti)]),
    "nfec_payload_id_length": (_I, [_U8]),
    "nfec_payload_id_write": (_I, [_U8, _U8, _U32, _U16, _U16, _P]),
    "nfec_payload_id_read": (_I, [_U8, _U8, _P, ctypes.POINTER(_U32), ctypes.POINTER(_U16), ctypes.POINTER(_U16)]),
    "nfec_sender_codec": (_I, [_U16, _U16, _U8, _I, ctypes.POINTER(_I), ctypes.POINTER(_U8), ctypes.POINTER(_U8)]),
    "nfec_receiver_codec": (_I, [_U8, _U8, _U16, _I, ctypes.POINTER(_I)]),
    "nfec_vector_size": (_U32, [_U16]),
    "nfec_npc_default_params": (None, [ctypes.POINTER(NpcParams)]),
    "nfec_npc_layout_for": (_I, [ctypes.POINTER(NpcParams), _U64, _I, ctypes.POINTER(NpcLayout)]),
    "nfec_npc_positions": (_I, [ctypes.POINTER(NpcLayout), _U64, _U64, _P]),
    "nfec_npc_encode_file": (_I, [_I, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(NpcParams)]),
    "nfec_npc_decode_file": (_I, [_I, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(NpcParams),
                                  ctypes.POINTER(_U64), ctypes.c_char_p, ctypes.c_size_t]),
    "nfec_npc_encode_file_multi": (_I, [_P, _I, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(NpcParams)]),
    "nfec_npc_decode_file_multi": (_I, [_P, _I, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(NpcParams),
                                        ctypes.POINTER(_U64), ctypes.c_char_p, ctypes.c_size_t]),
    "nfec_crc32_slots": (_I, [ctypes.POINTER(BlockBatch), _U32, _U32, _P, _P]),
}

_lib = None


def lib():
    """Load libnfec.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libnfec.so not built ({LIB_PATH}); run __graft_entry__.build() or make -C norm_amd")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    if _lib is None:
        return ""
    msg = _lib.nfec_last_error()
    return msg.decode() if msg else ""


def check(rc, what):
    if rc < 0:
        raise NfecError(rc, what)
    return rc


def stream_frame_workspace(n, capacity):
    """NFEC_STREAM_FRAME_WORKSPACE(n, capacity) of include/nfec.h, in bytes."""
    return (n + 2) * 40


def source_build_id(root=None):
    """SHA-256 of the library's sources in this tree, computed as norm_amd/Makefile computes
    nfec_build_id(): csrc/*.{cpp,hip,hpp,h} then include/*.h and include/norm_fec/*.h, each sorted by path."""
    import glob
    import hashlib

    root = root or os.path.dirname(_HERE)
    csrc = sorted(p for ext in ("cpp", "hip", "hpp", "h")
                  for p in glob.glob(os.path.join(root, "norm_amd", "csrc", "*." + ext)))
    inc = sorted(glob.glob(os.path.join(root, "include", "*.h")) + glob.glob(os.path.join(root, "include", "norm_fec", "*.h")))
    h = hashlib.sha256()
    for path in csrc + inc:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def declared_symbols():
    """Function names declared in include/nfec.h (used by the ABI export test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nfec_[a-z0-9_]+)\s*\(", text)))
