"""norm_amd -- MI355X-native Reed-Solomon FEC for NORM (RS8 / RS16 / MDP).

The hot path (parity generation and erasure repair over batches of FEC blocks) runs
as hand-written gfx950 HIP kernels in libnfec.so behind the C ABI of include/nfec.h.
This package is the Python mirror of the reference's NormEncoder/NormDecoder plugin
surface (include/normEncoder.h:38-54) plus batch entry points for device-resident data.
"""
from ._native import (NFEC_RS8, NFEC_RS16, NFEC_MDP, NFEC_ACCUMULATE, NFEC_FEATURE_RS16_TOEPLITZ,  # noqa: F401
                      NFEC_STREAM_EOM, NFEC_STREAM_FLUSH, NFEC_STREAM_END, NFEC_NACK_INFO, NFEC_TX_REPAIR_OBJECT, NFEC_TX_REPAIR_INFO,
                      NFEC_TX_PENDING_INFO, NFEC_DGRAM_UNREADABLE, NFEC_DGRAM_OTHER_TYPE, NFEC_DGRAM_MALFORMED,
                      NFEC_DGRAM_OTHER_SENDER, NFEC_DGRAM_OTHER_CODE, NFEC_DGRAM_OTHER_OBJECT, NFEC_DGRAM_REJECTED,
                      NFEC_DGRAM_DUPLICATE, NFEC_DGRAM_PLACED, NFEC_DGRAM_CLASSES, NFEC_DGRAM_PARSED, NFEC_CTL_UNREADABLE,
                      NFEC_CTL_OTHER_TYPE, NFEC_CTL_MALFORMED, NFEC_CTL_OTHER_FLAVOR, NFEC_CTL_OWN, NFEC_CTL_OTHER_SENDER,
                      NFEC_CTL_OTHER_INSTANCE, NFEC_CTL_NACK, NFEC_CTL_REPAIR_ADV, NFEC_CTL_CLASSES, NFEC_CTL_EXTENDED,
                      NFEC_CTL_ANY_INSTANCE, NFEC_CTL_TAKE_NACK, NFEC_CTL_TAKE_ADV, NfecError, lib)
from .codec import (  # noqa: F401
    NormEncoderRS8, NormDecoderRS8, NormEncoderRS16, NormDecoderRS16, NormEncoderMDP, NormDecoderMDP,
    BlockLayout, build_generator, device_count, fill_blocks, make_erasures, stream_copy, zero_erasures,
    received_mask, erasures_from_received_host, rx_parse_host, tx_list_host, rx_repair_requests_host,
    repair_parse_host, repair_max_units, repair_content_bound, object_layout, object_segment, object_block_sizes,
    StreamState, stream_frame_host, TxRepairState, tx_repair_state, tx_handle_nacks_host, tx_activate_repairs_host,
    tx_end_blocks_host, RxRepairState, rx_repair_state, rx_handle_repair_content_host, rx_repair_pending_host,
    tx_repair_adv_host, data_header, data_filter, data_header_bytes, data_header_write_host, rx_parse_data_host,
    rx_data_chunks_host, nack_header, adv_header, ctl_filter, nack_header_bytes, adv_header_bytes,
    nack_header_write_host, nack_fragment_host, adv_message_host, ctl_parse_host,
)

__version__ = "0.1.0"
