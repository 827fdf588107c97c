"""Python mirror of NORM's FEC plugin surface, backed by the MI355X kernels.

Class names, method names, argument meaning and return values follow the reference
classes (include/normEncoder.h:38-54, normEncoderRS8.h, normEncoderRS16.h,
normEncoderMDP.h) so parity tests read like the reference's own fecTest
(src/common/fecTest.cpp):

    enc = NormEncoderRS8(); enc.Init(numData, numParity, vectorSize)
    enc.Encode(segmentId, dataVector, parityVectorList)      # parity ^= G[k+i][seg] * data
    dec = NormDecoderRS8(); dec.Init(numData, numParity, vectorSize)
    dec.Decode(vectorList, numData, erasureCount, erasureLocs) -> erasureCount | 0

On top of the per-call surface, `encode_blocks` / `decode_blocks` take a batch of blocks
resident in HBM (a torch uint8 CUDA tensor shaped [nblocks, k+m, seg_stride]) -- the
performance path.  Everything runs through libnfec.so; nothing here computes.  The per-call
Encode / Decode follow the C++ drop-in's defaults: the library's host CPU paths
(nfec_encode_segment_host, and nfec_decode_vectors_host unless the repair is very large), with
host=False for the GPU round trip.
"""
import ctypes

from . import _native as N


def _addr_ro(buf):
    """Address of a read-only byte buffer (bytes, bytearray, numpy array, memoryview)."""
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data, buf
    if isinstance(buf, bytes):
        keep = ctypes.create_string_buffer(buf, len(buf))
        return ctypes.addressof(keep), keep
    mv = memoryview(buf)
    keep = (ctypes.c_char * mv.nbytes).from_buffer(mv)
    return ctypes.addressof(keep), keep


def _addr_rw(buf):
    if buf is None:
        return None, None
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data, buf
    mv = memoryview(buf)
    keep = (ctypes.c_char * mv.nbytes).from_buffer(mv)
    return ctypes.addressof(keep), keep


def _stream_handle(stream):
    if stream is not None:
        return ctypes.c_void_p(int(getattr(stream, "cuda_stream", stream)))
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tensor_ptr(t, what):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def device_count():
    return N.lib().nfec_device_count()


def build_generator(kind, num_data, num_parity):
    """Host-only generator parity rows (m x k) as a numpy array (no GPU needed)."""
    import numpy as np

    dtype = np.uint16 if kind == N.NFEC_RS16 else np.uint8
    out = np.zeros((num_parity, num_data), dtype)
    N.check(N.lib().nfec_build_generator(kind, num_data, num_parity, out.ctypes.data, out.nbytes),
            "nfec_build_generator")
    return out


class BlockLayout:
    """Contiguous HBM layout of a batch: block b, slot s at (b*(k+m) + s) * seg_stride."""

    def __init__(self, num_data, num_parity, vector_size, seg_stride=None):
        self.k, self.m, self.vec = num_data, num_parity, vector_size
        self.seg_stride = seg_stride or ((vector_size + 7) // 8 * 8)

    def empty(self, nblocks, device="cuda"):
        import torch

        return torch.zeros((nblocks, self.k + self.m, self.seg_stride), dtype=torch.uint8, device=device)


def _batch_struct(blocks, num_data, accumulate):
    if blocks.dtype.itemsize != 1 or blocks.dim() != 3:
        raise ValueError("blocks must be a uint8 tensor [nblocks, slots, seg_stride]")
    b = N.BlockBatch()
    b.blocks = blocks.data_ptr()
    b.block_stride = blocks.stride(0)
    b.seg_stride = blocks.stride(1)
    b.nblocks = blocks.shape[0]
    b.num_data = num_data.data_ptr() if num_data is not None else None
    b.flags = N.NFEC_ACCUMULATE if accumulate else 0
    if blocks.stride(2) != 1:
        raise ValueError("segment bytes must be contiguous")
    return b


class _Codec:
    """device: the GPU; devices: several GPUs (or one GPU listed several times) for one codec that
    stripes host batches over them (nfec_codec_create_ex); options: NFEC_OPT_* flags."""
    KIND = None

    def __init__(self, device=0, devices=None, options=0):
        self.device = device
        self.devices = list(devices) if devices else [device]
        self.options = options
        self._h = ctypes.c_void_p()
        self.ndata = self.npar = self.vector_size = 0

    # -- reference surface --
    def Init(self, numData, numParity, vectorSize):
        self.Destroy()
        cfg = N.CodecConfig()
        cfg.kind = self.KIND
        cfg.num_data, cfg.num_parity, cfg.vector_size = numData, numParity, vectorSize
        devs = (ctypes.c_int32 * len(self.devices))(*self.devices)
        cfg.devices = ctypes.cast(devs, ctypes.POINTER(ctypes.c_int32))
        cfg.num_devices = len(self.devices)
        cfg.flags = self.options
        rc = N.lib().nfec_codec_create_ex(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc == N.NFEC_ERANGE:
            return False  # reference: PLOG(PL_FATAL) + return false (normEncoderRS8.cpp:405-409)
        N.check(rc, "nfec_codec_create")
        self.ndata, self.npar, self.vector_size = numData, numParity, vectorSize
        return True

    def Destroy(self):
        if self._h:
            N.lib().nfec_codec_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass

    def GetNumData(self):
        return self.ndata

    def GetNumParity(self):
        return self.npar

    def GetVectorSize(self):
        return self.vector_size

    def num_devices(self):
        """The device ordinals the codec runs on (nfec_codec_num_devices)."""
        self._need()
        n = N.check(N.lib().nfec_codec_num_devices(self._h, None, 0), "nfec_codec_num_devices")
        out = (ctypes.c_int32 * n)()
        N.lib().nfec_codec_num_devices(self._h, out, n)
        return list(out)

    def generator(self):
        import numpy as np

        dtype = np.uint16 if self.KIND == N.NFEC_RS16 else np.uint8
        out = np.zeros((self.npar, self.ndata), dtype)
        N.check(N.lib().nfec_codec_get_generator(self._h, out.ctypes.data, out.nbytes), "nfec_codec_get_generator")
        return out

    def features(self):
        """Bit mask of the encode paths the codec chose (NFEC_FEATURE_*, include/nfec.h)."""
        self._need()
        rc = N.lib().nfec_codec_features(self._h)
        N.check(min(rc, 0), "nfec_codec_features")
        return rc

    def encode_paths(self):
        """Device-batch encodes so far per path that took them, {name: count} (NFEC_PATH_*,
        include/nfec.h): which kernel family a batch shape reaches."""
        self._need()
        cnt = (ctypes.c_uint64 * N.NFEC_PATH_COUNT)()
        rc = N.lib().nfec_codec_encode_paths(self._h, cnt, N.NFEC_PATH_COUNT)
        N.check(min(rc, 0), "nfec_codec_encode_paths")
        return {name: int(cnt[i]) for i, name in enumerate(N.PATH_NAMES)}

    def decode_paths(self):
        """Device-batch decodes so far per path that took them, {name: count} (NFEC_DPATH_*)."""
        self._need()
        cnt = (ctypes.c_uint64 * N.NFEC_DPATH_COUNT)()
        rc = N.lib().nfec_codec_decode_paths(self._h, cnt, N.NFEC_DPATH_COUNT)
        N.check(min(rc, 0), "nfec_codec_decode_paths")
        return {name: int(cnt[i]) for i, name in enumerate(N.DPATH_NAMES)}

    def tail_batches(self):
        """Device batches so far whose last vector_size % 8 bytes ran on the tail kernels beside
        the fast kernels, {"encode": n, "decode": n}."""
        self._need()
        cnt = (ctypes.c_uint64 * 2)()
        rc = N.lib().nfec_codec_tail_batches(self._h, cnt, 2)
        N.check(min(rc, 0), "nfec_codec_tail_batches")
        return {"encode": int(cnt[0]), "decode": int(cnt[1])}

    # -- receiver assembly on the device (nfec.h, "receiver assembly on the device") --
    def place_segments(self, blocks, received, payloads, offsets, block_index, symbol_id, length, num_data=None,
                       stats=None, stream=None):
        """Put received segments into their (block, slot) of a device batch (nfec_rx_place).
        received: the batch's reception mask (received_mask()); payloads: uint8 tensor holding the
        payload bytes; per segment i (all CUDA tensors of one length): offsets int64 (byte offset
        of its payload), block_index int32, symbol_id int16/uint16, length int16/uint16 (payload
        bytes, the rest of the slot up to vector_size becomes zero).  stats: int32 [3] the placed,
        duplicate and rejected counts are added to (zero it first), or None."""
        self._need()
        b = _batch_struct(blocks, num_data, False)
        _mask_check(received, blocks.shape[0])
        count = offsets.numel()
        for t, size, what in ((offsets, 8, "offsets"), (block_index, 4, "block_index"), (symbol_id, 2, "symbol_id"),
                              (length, 2, "length")):
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 3):
            raise ValueError("stats must hold three 32-bit counters")
        seg = N.RxSegments()
        seg.payloads = payloads.data_ptr() if payloads.numel() else None
        for name, t in (("offsets", offsets), ("block_index", block_index), ("symbol_id", symbol_id),
                        ("length", length)):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous CUDA (HIP) tensor")
            setattr(seg, name, t.data_ptr())
        if not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous CUDA (HIP) tensor")
        seg.count = count
        N.check(N.lib().nfec_rx_place(self._h, ctypes.byref(b), ctypes.byref(seg), _tensor_ptr(received, "received"),
                                      received.shape[1], _tensor_ptr(stats, "stats"), _stream_handle(stream)),
                "nfec_rx_place")

    def ingest_messages(self, blocks, received, payloads, offsets, length, fec_id, fec_m=8, first_block_id=0,
                        count_dev=None, num_data=None, block_index_out=None, symbol_id_out=None, stats=None,
                        stream=None):
        """place_segments with (block, slot) read on the device from the FEC payload ID in front of
        each payload (nfec_rx_ingest).  payloads: the wire buffer, a uint8 tensor; offsets int64 /
        length int16 per message, as list_pending returns them; fec_id / fec_m: the ID's form (5; 2
        with 8 or 16; 129); first_block_id: the block ID of the batch's block 0.  count_dev: a
        one-element int64 CUDA tensor (block_start[nblocks, :1]) that bounds the messages processed,
        or None.  block_index_out int32 / symbol_id_out int16: tensors of one element per message
        that receive what was parsed (all ones for a message outside the buffer), or None.  stats:
        as place_segments."""
        self._need()
        b = _batch_struct(blocks, num_data, False)
        _mask_check(received, blocks.shape[0])
        count = offsets.numel()
        given = [(offsets, 8, "offsets"), (length, 2, "length")]
        given += [(t, size, what) for t, size, what in ((block_index_out, 4, "block_index_out"),
                                                        (symbol_id_out, 2, "symbol_id_out")) if t is not None]
        for t, size, what in given:
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 3):
            raise ValueError("stats must hold three 32-bit counters")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        msg = N.RxMessages()
        msg.payloads = payloads.data_ptr() if payloads.numel() else None
        msg.payload_bytes = payloads.numel()
        msg.offsets, msg.length = offsets.data_ptr(), length.data_ptr()
        msg.count = count
        msg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        N.check(N.lib().nfec_rx_ingest(self._h, ctypes.byref(b), ctypes.byref(msg), fec_id, fec_m,
                                       first_block_id & 0xFFFFFFFF, _tensor_ptr(received, "received"),
                                       received.shape[1], _tensor_ptr(block_index_out, "block_index_out"),
                                       _tensor_ptr(symbol_id_out, "symbol_id_out"), _tensor_ptr(stats, "stats"),
                                       _stream_handle(stream)), "nfec_rx_ingest")

    def erasures_from_received(self, received, num_data=None, stride=None, stream=None):
        """The erasure lists decode_blocks takes, from a reception mask (nfec_rx_erasures):
        (locs int16 [nblocks, stride], counts int16 [nblocks]); stride defaults to numParity.
        counts holds the full number of erasures even past stride."""
        import torch

        self._need()
        _mask_check(received, received.shape[0])
        nb = received.shape[0]
        stride = self.npar if stride is None else stride
        locs = torch.zeros((nb, stride), dtype=torch.int16, device=received.device)
        counts = torch.zeros(nb, dtype=torch.int16, device=received.device)
        N.check(N.lib().nfec_rx_erasures(self._h, _tensor_ptr(received, "received"), received.shape[1],
                                         _tensor_ptr(num_data, "num_data"), nb, _tensor_ptr(locs, "locs"), stride,
                                         _tensor_ptr(counts, "counts"), _stream_handle(stream)), "nfec_rx_erasures")
        return locs, counts

    def repair_requests(self, received, num_data=None, fec_id=5, fec_m=8, object_id=0, first_block_id=0, flags=0,
                        max_units=None, capacity=None, content=None, stream=None):
        """The repair-request content of a NORM_NACK from a reception mask (nfec_rx_repair_requests):
        (content uint8 [capacity], block_start int64 [nblocks + 1, 2], totals int64 [4]).  totals =
        (bytes, requests, needing blocks, absent blocks), the full numbers even past capacity;
        block_start[b] = (offset of what is emitted at block b's position, the block's class 0 / 1 / 2
        for silent / needing / absent).  max_units defaults to the most a request may hold;
        capacity to what every block's longest content needs (`content`: a uint8 tensor to write
        into instead, 4-byte aligned).  The mask is only read."""
        import torch

        self._need()
        _mask_check(received, received.shape[0])
        nb = received.shape[0]
        max_units = repair_max_units(fec_id) if max_units is None else max_units
        if content is None:
            capacity = repair_content_bound(self.ndata, self.npar, nb, fec_id) if capacity is None else capacity
            content = torch.zeros(capacity, dtype=torch.uint8, device=received.device)
        capacity = content.numel() if capacity is None else capacity
        block_start = torch.zeros((nb + 1, 2), dtype=torch.int64, device=received.device)
        totals = torch.zeros(4, dtype=torch.int64, device=received.device)
        N.check(N.lib().nfec_rx_repair_requests(self._h, _tensor_ptr(received, "received"), received.shape[1],
                                                _tensor_ptr(num_data, "num_data"), nb, fec_id, fec_m, object_id & 0xFFFF,
                                                first_block_id & 0xFFFFFFFF, flags, max_units,
                                                _tensor_ptr(content, "content"), capacity,
                                                _tensor_ptr(block_start, "block_start"), _tensor_ptr(totals, "totals"),
                                                _stream_handle(stream)), "nfec_rx_repair_requests")
        return content, block_start, totals

    # -- sender assembly on the device (nfec.h, "sender assembly on the device") --
    def list_pending(self, pending, num_data=None, seg_length=None, gap=0, capacity=None, stream=None):
        """The transmission list of a pending mask (nfec_tx_list), in NextSenderMsg's order:
        (offsets int64, block_index int32, symbol_id int16, length int16, block_start int64
        [nblocks + 1, 2]).  pending: 32-bit tensor [nblocks, mask_stride]; seg_length: 16-bit
        tensor [nblocks, >= k] of the source segments' lengths, or None (all vector_size); gap:
        bytes left free in front of every payload.  The four arrays hold `capacity` entries
        (default: every slot of every block); block_start[nblocks] = (entries, wire bytes) is the
        full total even past capacity, and block_start[nblocks, :1] is emit_segments' count_dev."""
        import torch

        self._need()
        _mask_check(pending, pending.shape[0])
        nb = pending.shape[0]
        capacity = nb * (self.ndata + self.npar) if capacity is None else capacity
        lstride = 0
        if seg_length is not None:
            if seg_length.dim() != 2 or seg_length.element_size() != 2 or seg_length.shape[0] != nb:
                raise ValueError("seg_length must be a 16-bit tensor [nblocks, length_stride]")
            lstride = seg_length.shape[1]
        dev = pending.device
        offsets = torch.zeros(capacity, dtype=torch.int64, device=dev)
        block_index = torch.zeros(capacity, dtype=torch.int32, device=dev)
        symbol_id = torch.zeros(capacity, dtype=torch.int16, device=dev)
        length = torch.zeros(capacity, dtype=torch.int16, device=dev)
        block_start = torch.zeros((nb + 1, 2), dtype=torch.int64, device=dev)
        N.check(N.lib().nfec_tx_list(self._h, _tensor_ptr(pending, "pending"), pending.shape[1],
                                     _tensor_ptr(num_data, "num_data"), nb, _tensor_ptr(seg_length, "seg_length"),
                                     lstride, gap, _tensor_ptr(offsets, "offsets"),
                                     _tensor_ptr(block_index, "block_index"), _tensor_ptr(symbol_id, "symbol_id"),
                                     _tensor_ptr(length, "length"), capacity, _tensor_ptr(block_start, "block_start"),
                                     _stream_handle(stream)), "nfec_tx_list")
        return offsets, block_index, symbol_id, length, block_start

    def emit_segments(self, blocks, payloads, offsets, block_index, symbol_id, length, count_dev=None, fec_id=0,
                      fec_m=8, first_block_id=0, pending=None, num_data=None, stats=None, stream=None):
        """Write the listed slots of a device batch into the wire buffer `payloads` (uint8 tensor),
        each behind its FEC payload ID (nfec_tx_emit; fec_id 0: no ID).  The four descriptor tensors
        are list_pending's; count_dev: a one-element int64 CUDA tensor (block_start[nblocks, :1])
        that bounds the entries processed, or None.  pending: the mask whose bits are cleared, or
        None.  stats: int32 [2] the emitted and rejected counts are added to (zero it first), or
        None."""
        self._need()
        b = _batch_struct(blocks, num_data, False)
        if pending is not None:
            _mask_check(pending, blocks.shape[0])
        count = offsets.numel()
        for t, size, what in ((offsets, 8, "offsets"), (block_index, 4, "block_index"), (symbol_id, 2, "symbol_id"),
                              (length, 2, "length")):
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 2):
            raise ValueError("stats must hold two 32-bit counters")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        seg = N.TxSegments()
        seg.payloads = payloads.data_ptr() if payloads.numel() else None
        seg.payload_bytes = payloads.numel()
        seg.offsets, seg.block_index = offsets.data_ptr(), block_index.data_ptr()
        seg.symbol_id, seg.length = symbol_id.data_ptr(), length.data_ptr()
        seg.count = count
        seg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        N.check(N.lib().nfec_tx_emit(self._h, ctypes.byref(b), ctypes.byref(seg), fec_id, fec_m,
                                     first_block_id & 0xFFFFFFFF, _tensor_ptr(pending, "pending"),
                                     pending.shape[1] if pending is not None else 0, _tensor_ptr(stats, "stats"),
                                     _stream_handle(stream)), "nfec_tx_emit")

    # -- NORM_DATA messages on the device (nfec.h, "NORM_DATA messages on the device") --
    def emit_data_messages(self, blocks, payloads, offsets, block_index, symbol_id, length, header, count_dev=None,
                           first_block_id=0, pending=None, num_data=None, msg_offsets_out=None, msg_length_out=None,
                           stats=None, stream=None):
        """emit_segments with the whole NORM_DATA header in front of every payload (nfec_tx_emit_data).
        header: data_header(...); the four descriptor tensors are list_pending's, built with gap =
        data_header_bytes(header.fec_id, header.ext_bytes).  msg_offsets_out int64 / msg_length_out
        int16: tensors of one element per entry that receive each datagram's start and length (0 / 0
        for a rejected entry), the table ingest_datagrams takes, or None.  The rest as emit_segments."""
        self._need()
        b = _batch_struct(blocks, num_data, False)
        if pending is not None:
            _mask_check(pending, blocks.shape[0])
        count = offsets.numel()
        given = [(offsets, 8, "offsets"), (block_index, 4, "block_index"), (symbol_id, 2, "symbol_id"),
                 (length, 2, "length")]
        given += [(t, size, what) for t, size, what in ((msg_offsets_out, 8, "msg_offsets_out"),
                                                        (msg_length_out, 2, "msg_length_out")) if t is not None]
        for t, size, what in given:
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 2):
            raise ValueError("stats must hold two 32-bit counters")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        seg = N.TxSegments()
        seg.payloads = payloads.data_ptr() if payloads.numel() else None
        seg.payload_bytes = payloads.numel()
        seg.offsets, seg.block_index = offsets.data_ptr(), block_index.data_ptr()
        seg.symbol_id, seg.length = symbol_id.data_ptr(), length.data_ptr()
        seg.count = count
        seg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        N.check(N.lib().nfec_tx_emit_data(self._h, ctypes.byref(b), ctypes.byref(seg), ctypes.byref(header),
                                          first_block_id & 0xFFFFFFFF, _tensor_ptr(pending, "pending"),
                                          pending.shape[1] if pending is not None else 0,
                                          _tensor_ptr(msg_offsets_out, "msg_offsets_out"),
                                          _tensor_ptr(msg_length_out, "msg_length_out"), _tensor_ptr(stats, "stats"),
                                          _stream_handle(stream)), "nfec_tx_emit_data")

    def ingest_datagrams(self, blocks, received, payloads, offsets, length, filter, first_block_id=0, count_dev=None,
                         num_data=None, class_out=None, sequence_out=None, block_index_out=None, symbol_id_out=None,
                         stats=None, totals=None, stream=None):
        """ingest_messages on raw NORM_DATA datagrams (nfec_rx_ingest_data): offsets int64 / length
        int16 are each datagram's start and length in the wire buffer `payloads`; filter:
        data_filter(...).  class_out uint8 / sequence_out int16 / block_index_out int32 /
        symbol_id_out int16: tensors of one element per datagram, or None.  stats: int32 [9], one
        counter per NFEC_DGRAM_* class (zero it first), or None.  totals: int64 [1] set to -1 by the
        caller, receives the smallest index of a datagram past the filter that carries an FTI, or
        None."""
        self._need()
        b = _batch_struct(blocks, num_data, False)
        _mask_check(received, blocks.shape[0])
        count = offsets.numel()
        given = [(offsets, 8, "offsets"), (length, 2, "length")]
        given += [(t, size, what) for t, size, what in ((class_out, 1, "class_out"), (sequence_out, 2, "sequence_out"),
                                                        (block_index_out, 4, "block_index_out"),
                                                        (symbol_id_out, 2, "symbol_id_out")) if t is not None]
        for t, size, what in given:
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < N.NFEC_DGRAM_CLASSES):
            raise ValueError("stats must hold nine 32-bit counters")
        if totals is not None and (totals.element_size() != 8 or totals.numel() < 1):
            raise ValueError("totals must hold one 64-bit value")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        msg = N.RxMessages()
        msg.payloads = payloads.data_ptr() if payloads.numel() else None
        msg.payload_bytes = payloads.numel()
        msg.offsets, msg.length = offsets.data_ptr(), length.data_ptr()
        msg.count = count
        msg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        N.check(N.lib().nfec_rx_ingest_data(self._h, ctypes.byref(b), ctypes.byref(msg), ctypes.byref(filter),
                                            first_block_id & 0xFFFFFFFF, _tensor_ptr(received, "received"),
                                            received.shape[1], _tensor_ptr(class_out, "class_out"),
                                            _tensor_ptr(sequence_out, "sequence_out"),
                                            _tensor_ptr(block_index_out, "block_index_out"),
                                            _tensor_ptr(symbol_id_out, "symbol_id_out"), _tensor_ptr(stats, "stats"),
                                            _tensor_ptr(totals, "totals"), _stream_handle(stream)),
                "nfec_rx_ingest_data")

    # -- NORM_NACK and REPAIR_ADV messages on the device (nfec.h, "NORM_NACK and NORM_CMD(REPAIR_ADV) messages ...") --
    def nack_messages(self, content, content_bytes_dev, header, segment_size, fec_id=5, block_start=None, wire=None,
                      pitch=None, capacity=None, msg_offsets_out=None, msg_length_out=None, totals=None, workspace=None,
                      stream=None):
        """Repair-request content cut into whole NORM_NACK messages (nfec_nack_fragment).  content:
        repair_requests' uint8 tensor; content_bytes_dev: its totals[:1] (a one-element int64 CUDA
        tensor); block_start: repair_requests' second result, the hint that makes the request index
        parallel, or None (correct, but one lane walks every request header).  header:
        nack_header(...).  Message i lies at wire[i * pitch:]; pitch defaults to header +
        segment_size, capacity to what `wire` holds or, with wire None, to what the content could
        need.  Returns (wire uint8, msg_offsets int64 [capacity], msg_length int16 [capacity],
        totals int64 [6] = (messages, content bytes written, requests read, requests split, content
        bytes consumed, cut short)); totals[:1] is the count_dev of ingest_control and handle_nacks."""
        import torch

        self._need()
        if content.element_size() != 1 or not content.is_cuda or not content.is_contiguous():
            raise ValueError("content must be a contiguous uint8 CUDA (HIP) tensor")
        if content_bytes_dev.element_size() != 8 or content_bytes_dev.numel() < 1 or not content_bytes_dev.is_cuda:
            raise ValueError("content_bytes_dev must be a 64-bit CUDA (HIP) tensor")
        dev = content.device
        H = nack_header_bytes(header.ext_bytes)
        pitch = H + segment_size if pitch is None else pitch
        if wire is None:
            if capacity is None:
                capacity = content.numel() // max(segment_size - 64, 8) + 2
            wire = torch.zeros(max(capacity * pitch, 4), dtype=torch.uint8, device=dev)
        if capacity is None:
            capacity = wire.numel() // pitch if pitch else 0
        nb = 0
        if block_start is not None:
            if block_start.element_size() != 8 or block_start.dim() != 2 or block_start.shape[1] != 2:
                raise ValueError("block_start must be a 64-bit tensor [nblocks + 1, 2]")
            nb = block_start.shape[0] - 1
        if msg_offsets_out is None:
            msg_offsets_out = torch.zeros(capacity, dtype=torch.int64, device=dev)
        if msg_length_out is None:
            msg_length_out = torch.zeros(capacity, dtype=torch.int16, device=dev)
        for t, size, what in ((msg_offsets_out, 8, "msg_offsets_out"), (msg_length_out, 2, "msg_length_out")):
            if t.element_size() != size or t.numel() < capacity or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor of {capacity} elements of {size} bytes")
        if totals is None:
            totals = torch.zeros(6, dtype=torch.int64, device=dev)
        need = N.lib().nfec_nack_fragment_workspace_bytes(content.numel(), nb)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        N.check(N.lib().nfec_nack_fragment(self._h, _tensor_ptr(content, "content"), content.numel(),
                                           content_bytes_dev.data_ptr(), _tensor_ptr(block_start, "block_start"), nb,
                                           fec_id, segment_size, ctypes.byref(header), _tensor_ptr(wire, "wire"),
                                           wire.numel(), pitch, _tensor_ptr(msg_offsets_out, "msg_offsets_out"),
                                           _tensor_ptr(msg_length_out, "msg_length_out"), capacity,
                                           _tensor_ptr(totals, "totals"), _tensor_ptr(workspace, "workspace"),
                                           workspace.numel(), _stream_handle(stream)), "nfec_nack_fragment")
        return wire, msg_offsets_out, msg_length_out, totals

    def repair_adv_message(self, content, content_bytes_dev, header, segment_size, fec_id=5, wire=None, stream=None):
        """One NORM_CMD(REPAIR_ADV) from repair_adv's content (nfec_tx_repair_adv_message): the
        header, then the first message of nack_messages' cut; the LIMIT flag is set when content
        remained.  header: adv_header(...).  Returns (wire uint8, msg_length int16 [1], totals int64
        [3] = (content bytes written, content bytes left out, limit flag))."""
        import torch

        self._need()
        if content.element_size() != 1 or not content.is_cuda or not content.is_contiguous():
            raise ValueError("content must be a contiguous uint8 CUDA (HIP) tensor")
        if content_bytes_dev.element_size() != 8 or content_bytes_dev.numel() < 1 or not content_bytes_dev.is_cuda:
            raise ValueError("content_bytes_dev must be a 64-bit CUDA (HIP) tensor")
        dev = content.device
        if wire is None:
            wire = torch.zeros(adv_header_bytes(header.ext_bytes) + segment_size, dtype=torch.uint8, device=dev)
        msg_length = torch.zeros(1, dtype=torch.int16, device=dev)
        totals = torch.zeros(3, dtype=torch.int64, device=dev)
        N.check(N.lib().nfec_tx_repair_adv_message(self._h, _tensor_ptr(content, "content"), content.numel(),
                                                   content_bytes_dev.data_ptr(), fec_id, segment_size,
                                                   ctypes.byref(header), _tensor_ptr(wire, "wire"), wire.numel(),
                                                   _tensor_ptr(msg_length, "msg_length"), _tensor_ptr(totals, "totals"),
                                                   _stream_handle(stream)), "nfec_tx_repair_adv_message")
        return wire, msg_length, totals

    def ingest_control(self, payloads, offsets, length, filter, count_dev=None, class_out=None, source_id_out=None,
                       grtt_response_out=None, stats=None, stream=None):
        """The intake for control datagrams (nfec_rx_ingest_control): offsets int64 / length int16
        are each datagram's start and length in the wire buffer `payloads`; filter:
        ctl_filter(...).  Returns (content_offset int64, content_length int16), index-aligned with
        the datagrams: the arrays handle_nacks and handle_repair_content take with the same
        payloads; a datagram that is not taken is the empty message (0, 0).  class_out uint8 /
        source_id_out int32 / grtt_response_out int32 [count, 2]: tensors, or None.  stats: int32
        [9], one counter per NFEC_CTL_* class (zero it first), or None."""
        import torch

        self._need()
        count = offsets.numel()
        given = [(offsets, 8, count, "offsets"), (length, 2, count, "length")]
        given += [(t, size, n, what) for t, size, n, what in ((class_out, 1, count, "class_out"),
                                                              (source_id_out, 4, count, "source_id_out"),
                                                              (grtt_response_out, 4, 2 * count, "grtt_response_out"))
                  if t is not None]
        for t, size, n, what in given:
            if t.element_size() != size or t.numel() != n:
                raise ValueError(f"{what} must hold {n} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < N.NFEC_CTL_CLASSES):
            raise ValueError("stats must hold nine 32-bit counters")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        content_offset = torch.zeros(count, dtype=torch.int64, device=payloads.device)
        content_length = torch.zeros(count, dtype=torch.int16, device=payloads.device)
        msg = N.RxMessages()
        msg.payloads = payloads.data_ptr() if payloads.numel() else None
        msg.payload_bytes = payloads.numel()
        msg.offsets, msg.length = offsets.data_ptr(), length.data_ptr()
        msg.count = count
        msg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        N.check(N.lib().nfec_rx_ingest_control(self._h, ctypes.byref(msg), ctypes.byref(filter),
                                               _tensor_ptr(class_out, "class_out"),
                                               _tensor_ptr(content_offset, "content_offset"),
                                               _tensor_ptr(content_length, "content_length"),
                                               _tensor_ptr(source_id_out, "source_id_out"),
                                               _tensor_ptr(grtt_response_out, "grtt_response_out"),
                                               _tensor_ptr(stats, "stats"), _stream_handle(stream)),
                "nfec_rx_ingest_control")
        return content_offset, content_length

    # -- sender repair state on the device (nfec.h, "sender repair state on the device") --
    def handle_nacks(self, state, payloads, offsets, length, num_data=None, fec_id=5, fec_m=8, object_id=0,
                     first_block_id=0, extra_parity=0, unit_capacity=None, count_dev=None, workspace=None,
                     totals=None, stream=None):
        """The NACKs of a repair cycle into the sender's repair state (nfec_tx_handle_nacks:
        SenderHandleNackMessage, !holdoff, for one object).  state: tx_repair_state(..., device=...);
        payloads: the wire buffer, a uint8 tensor; message i is the repair-request content
        payloads[offsets[i] : offsets[i] + length[i]] of one NORM_NACK (offsets int64, length int16,
        handled in index order).  unit_capacity bounds the units of the call (default: what the
        buffer's bytes could hold); when they exceed it nothing is changed.  workspace: a uint8
        tensor of handle_nacks_workspace_bytes() bytes, or None.  Returns totals int64 [6] = (units,
        SEGMENT units applied, units not applied or ignored, block_repair bits newly set, messages
        cut short, messages unreadable)."""
        import torch

        self._need()
        count = offsets.numel()
        for t, size, what in ((offsets, 8, "offsets"), (length, 2, "length")):
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        nb = state.nblocks
        if unit_capacity is None:
            unit_capacity = payloads.numel() // 8 + 1
        need = N.lib().nfec_tx_nack_workspace_bytes(unit_capacity, count, nb)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=payloads.device)
        if totals is None:
            totals = torch.zeros(6, dtype=torch.int64, device=payloads.device)
        msg = N.RxMessages()
        msg.payloads = payloads.data_ptr() if payloads.numel() else None
        msg.payload_bytes = payloads.numel()
        msg.offsets, msg.length = offsets.data_ptr(), length.data_ptr()
        msg.count = count
        msg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        st = state.struct()
        N.check(N.lib().nfec_tx_handle_nacks(self._h, ctypes.byref(msg), fec_id, fec_m, object_id & 0xFFFF,
                                             first_block_id & 0xFFFFFFFF, _tensor_ptr(num_data, "num_data"), nb,
                                             state.mask_stride, extra_parity, ctypes.byref(st), unit_capacity,
                                             _tensor_ptr(workspace, "workspace"), workspace.numel(),
                                             _tensor_ptr(totals, "totals"), _stream_handle(stream)),
                "nfec_tx_handle_nacks")
        return totals

    def activate_repairs(self, state, pending, num_data=None, auto_parity=0, totals=None, stream=None):
        """What the handled NACKs left in the repair state into the pending mask
        (nfec_tx_activate_repairs: OnRepairTimeout for the object).  Returns totals int64 [3] = (blocks
        reset with a change, blocks whose segment repairs were activated, pending bits after)."""
        import torch

        self._need()
        _mask_check(pending, state.nblocks)
        if pending.shape[1] != state.mask_stride:
            raise ValueError("pending and state.repair must have one mask_stride")
        if totals is None:
            totals = torch.zeros(3, dtype=torch.int64, device=pending.device)
        st = state.struct()
        N.check(N.lib().nfec_tx_activate_repairs(self._h, _tensor_ptr(num_data, "num_data"), state.nblocks, auto_parity,
                                                 _tensor_ptr(pending, "pending"), state.mask_stride, ctypes.byref(st),
                                                 _tensor_ptr(totals, "totals"), _stream_handle(stream)),
                "nfec_tx_activate_repairs")
        return totals

    def end_blocks(self, state, pending, num_data=None, stream=None):
        """NextSenderMsg's end of block (nfec_tx_end_blocks): a block whose pending mask is empty
        moves its parity_count into its parity_offset.  After emit_segments, before the next
        handle_nacks."""
        self._need()
        _mask_check(pending, state.nblocks)
        if pending.shape[1] != state.mask_stride:
            raise ValueError("pending and state.repair must have one mask_stride")
        st = state.struct()
        N.check(N.lib().nfec_tx_end_blocks(self._h, _tensor_ptr(num_data, "num_data"), state.nblocks,
                                           _tensor_ptr(pending, "pending"), state.mask_stride, ctypes.byref(st),
                                           _stream_handle(stream)), "nfec_tx_end_blocks")

    # -- NACK suppression and repair advertisements (nfec.h, "NACK suppression and repair advertisements on the device") --
    def rx_repair_state(self, nblocks, k=None, m=None, device=None):
        """A zeroed suppression state (RxRepairState) for nblocks blocks of k + m slots (default: this
        codec's) on `device` (default: the codec's first)."""
        self._need()
        return rx_repair_state(nblocks, self.ndata if k is None else k, self.npar if m is None else m,
                               device=f"cuda:{self.device}" if device is None else device)

    def handle_repair_content(self, state, received, payloads, offsets, length, num_data=None, fec_id=5, fec_m=8,
                              object_id=0, first_block_id=0, count_dev=None, totals=None, stream=None):
        """Overheard repair-request content into a receiver's suppression state
        (nfec_rx_handle_repair_content: HandleRepairContent for one object).  state:
        rx_repair_state(...); received: the receiver's reception mask, only read; message i is
        payloads[offsets[i] : offsets[i] + length[i]], the content of one NORM_NACK or REPAIR_ADV
        (offsets int64, length int16).  Returns totals int64 [6] = (units, SEGMENT units applied,
        units not applied or ignored, block_repair bits newly set, messages cut short, messages
        unreadable)."""
        import torch

        self._need()
        _mask_check(received, state.nblocks)
        if received.shape[1] != state.mask_stride:
            raise ValueError("received and state.repair must have one mask_stride")
        count = offsets.numel()
        for t, size, what in ((offsets, 8, "offsets"), (length, 2, "length")):
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"{what} must hold {count} elements of {size} bytes")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        if payloads.element_size() != 1 or not payloads.is_cuda or not payloads.is_contiguous():
            raise ValueError("payloads must be a contiguous uint8 CUDA (HIP) tensor")
        if totals is None:
            totals = torch.zeros(6, dtype=torch.int64, device=payloads.device)
        msg = N.RxMessages()
        msg.payloads = payloads.data_ptr() if payloads.numel() else None
        msg.payload_bytes = payloads.numel()
        msg.offsets, msg.length = offsets.data_ptr(), length.data_ptr()
        msg.count = count
        msg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        st = state.struct()
        N.check(N.lib().nfec_rx_handle_repair_content(self._h, ctypes.byref(msg), fec_id, fec_m, object_id & 0xFFFF,
                                                      first_block_id & 0xFFFFFFFF, _tensor_ptr(received, "received"),
                                                      state.mask_stride, _tensor_ptr(num_data, "num_data"), state.nblocks,
                                                      ctypes.byref(st), _tensor_ptr(totals, "totals"),
                                                      _stream_handle(stream)), "nfec_rx_handle_repair_content")
        return totals

    def repair_pending(self, state, received, num_data=None, flags=0, pending_blocks=None, totals=None, stream=None):
        """The decision at the end of the back-off (nfec_rx_repair_pending).  Returns (totals int64 [4]
        = (send, blocks pending, needing blocks suppressed, absent blocks suppressed), pending_blocks
        int32 [(nblocks + 31) // 32]: bit b % 32 of word b // 32 is block b).  The state is only read."""
        import torch

        self._need()
        _mask_check(received, state.nblocks)
        if received.shape[1] != state.mask_stride:
            raise ValueError("received and state.repair must have one mask_stride")
        if pending_blocks is None:
            pending_blocks = torch.empty(max(1, (state.nblocks + 31) // 32), dtype=torch.int32, device=received.device)
        if totals is None:
            totals = torch.zeros(4, dtype=torch.int64, device=received.device)
        st = state.struct()
        N.check(N.lib().nfec_rx_repair_pending(self._h, _tensor_ptr(received, "received"), state.mask_stride,
                                               _tensor_ptr(num_data, "num_data"), state.nblocks, ctypes.byref(st), flags,
                                               _tensor_ptr(pending_blocks, "pending_blocks"), _tensor_ptr(totals, "totals"),
                                               _stream_handle(stream)), "nfec_rx_repair_pending")
        return totals, pending_blocks

    def repair_adv(self, state, num_data=None, fec_id=5, fec_m=8, object_id=0, first_block_id=0, max_units=None,
                   capacity=None, content=None, stream=None):
        """The repair-request content of a NORM_CMD(REPAIR_ADV) from the sender's repair state
        (nfec_tx_repair_adv), behind handle_nacks and before activate_repairs: (content uint8
        [capacity], block_start int64 [nblocks + 1, 2], totals int64 [4]) as repair_requests, with
        totals = (bytes, requests, blocks with segment requests, whole blocks).  The state is only
        read."""
        import torch

        self._need()
        nb = state.nblocks
        dev = state.repair.device
        max_units = repair_max_units(fec_id) if max_units is None else max_units
        if content is None:
            capacity = repair_content_bound(self.ndata, self.npar, nb, fec_id) if capacity is None else capacity
            content = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        capacity = content.numel() if capacity is None else capacity
        block_start = torch.zeros((nb + 1, 2), dtype=torch.int64, device=dev)
        totals = torch.zeros(4, dtype=torch.int64, device=dev)
        st = state.struct()
        N.check(N.lib().nfec_tx_repair_adv(self._h, ctypes.byref(st), state.mask_stride, _tensor_ptr(num_data, "num_data"),
                                           nb, fec_id, fec_m, object_id & 0xFFFF, first_block_id & 0xFFFFFFFF, max_units,
                                           _tensor_ptr(content, "content"), capacity,
                                           _tensor_ptr(block_start, "block_start"), _tensor_ptr(totals, "totals"),
                                           _stream_handle(stream)), "nfec_tx_repair_adv")
        return content, block_start, totals

    # -- object segmentation on the device (nfec.h, "object segmentation on the device") --
    def _object_call(self, obj, layout, blocks):
        self._need()
        if obj.element_size() != 1 or not obj.is_cuda or not obj.is_contiguous():
            raise ValueError("obj must be a contiguous uint8 CUDA (HIP) tensor")
        if not isinstance(layout, N.ObjectLayout):
            raise ValueError("layout must come from object_layout()")
        return _batch_struct(blocks, None, False)

    def read_object(self, obj, layout, blocks, first_block=0, num_data=None, seg_length=None, stream=None):
        """Fill the source slots of a device batch from a NORM data object in device memory
        (nfec_object_read: ReadSegment and CalculateBlockParity's zero pad).  obj: uint8 tensor that
        holds the object from its element 0 on, at any byte alignment; layout: object_layout();
        batch block i is object block first_block + i.  num_data: 16-bit tensor [nblocks] that
        receives the blocks' sizes (encode_blocks' num_data), or None; seg_length: 16-bit tensor
        [nblocks, >= k] that receives the source segments' lengths (list_pending's seg_length), or
        None.  Parity slots and stride padding keep their bytes."""
        b = self._object_call(obj, layout, blocks)
        lstride = 0
        if seg_length is not None:
            if seg_length.dim() != 2 or seg_length.element_size() != 2 or seg_length.shape[0] != blocks.shape[0]:
                raise ValueError("seg_length must be a 16-bit tensor [nblocks, length_stride]")
            lstride = seg_length.shape[1]
        if num_data is not None and (num_data.element_size() != 2 or num_data.numel() < blocks.shape[0]):
            raise ValueError("num_data must be a 16-bit tensor [nblocks]")
        N.check(N.lib().nfec_object_read(self._h, ctypes.byref(layout), _tensor_ptr(obj, "obj"), obj.numel(),
                                         first_block, ctypes.byref(b), _tensor_ptr(num_data, "num_data"),
                                         _tensor_ptr(seg_length, "seg_length"), lstride, _stream_handle(stream)),
                "nfec_object_read")

    def write_object(self, obj, layout, blocks, first_block=0, received=None, status=None, stats=None, stream=None):
        """Deliver source slots of a device batch to their bytes of a NORM data object in device
        memory (nfec_object_write: WriteSegment).  A segment is written when received is None, when
        its bit is set in the reception mask `received`, or when status (decode_received's int32
        [nblocks]) is positive for its block; obj.numel() bounds the writes as data_max does.  No
        other byte of obj changes.  stats: int32 [2] the selected and not-selected segment counts
        are added to (zero it first), or None."""
        b = self._object_call(obj, layout, blocks)
        if received is not None:
            _mask_check(received, blocks.shape[0])
        if status is not None and (status.element_size() != 4 or status.numel() < blocks.shape[0]):
            raise ValueError("status must be a 32-bit tensor [nblocks]")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 2):
            raise ValueError("stats must hold two 32-bit counters")
        N.check(N.lib().nfec_object_write(self._h, ctypes.byref(layout), _tensor_ptr(obj, "obj"), obj.numel(),
                                          first_block, ctypes.byref(b), _tensor_ptr(received, "received"),
                                          received.shape[1] if received is not None else 0,
                                          _tensor_ptr(status, "status"), _tensor_ptr(stats, "stats"),
                                          _stream_handle(stream)), "nfec_object_write")

    # -- stream objects on the device (nfec.h, "stream objects on the device") --
    def frame_stream(self, write_len, write_flags, state, segment_size=None, capacity=None, stream=None):
        """Frame application writes of a NORM stream into segments on the device (nfec_stream_frame:
        NormStreamObject::Write's loop).  write_len: 32-bit CUDA tensor [n]; write_flags: uint8
        tensor [n] of NFEC_STREAM_EOM / NFEC_STREAM_FLUSH; state: the StreamState the calls before
        left (host values).  Returns (seg_start int64, seg_len int16, seg_msg_start int16, totals
        int64 [4], state_out): the three tables hold `capacity` entries (it must be given unless
        there are no writes: how many segments the writes close is not known on the host),
        totals = (segments, bytes consumed, carry bytes, carry_msg_start) and state_out is a uint8
        tensor that holds the advanced nfec_stream_state (StreamState.from_tensor reads it).
        totals[:1] is pack_stream's count_dev."""
        import torch

        self._need()
        n = write_len.numel()
        if n and (write_len.element_size() != 4 or write_flags.element_size() != 1 or write_flags.numel() != n):
            raise ValueError("write_len must hold 32-bit lengths and write_flags as many bytes")
        if capacity is None:
            if n:
                raise ValueError("capacity must be given")
            capacity = 0
        S = self.vector_size - 8 if segment_size is None else segment_size
        dev = write_len.device
        seg_start = torch.zeros(capacity, dtype=torch.int64, device=dev)
        seg_len = torch.zeros(capacity, dtype=torch.int16, device=dev)
        seg_ms = torch.zeros(capacity, dtype=torch.int16, device=dev)
        totals = torch.zeros(4, dtype=torch.int64, device=dev)
        state_out = torch.zeros(ctypes.sizeof(N.StreamState), dtype=torch.uint8, device=dev)
        ws = torch.empty(N.stream_frame_workspace(n, capacity) // 8, dtype=torch.int64, device=dev)
        N.check(N.lib().nfec_stream_frame(self._h, S, _tensor_ptr(write_len, "write_len") if n else None,
                                          _tensor_ptr(write_flags, "write_flags") if n else None, n, state,
                                          _tensor_ptr(state_out, "state_out"), _tensor_ptr(seg_start, "seg_start"),
                                          _tensor_ptr(seg_len, "seg_len"), _tensor_ptr(seg_ms, "seg_msg_start"), capacity,
                                          _tensor_ptr(totals, "totals"), _tensor_ptr(ws, "workspace"),
                                          _stream_handle(stream)), "nfec_stream_frame")
        return seg_start, seg_len, seg_ms, totals, state_out

    def pack_stream(self, data, seg_start, seg_len, seg_msg_start, blocks, first_slot=0, write_offset=0, count_dev=None,
                    end=False, segment_size=None, num_data=None, seg_length=None, stats=None, stream=None):
        """Put framed segments of a stream into the source slots of a device batch (nfec_stream_pack):
        the 8-byte stream payload header, the segment's bytes of `data` (uint8 CUDA tensor: the
        byte run the table was framed over, at any alignment), zeros up to vector_size.  Entry i
        goes to stream slot first_slot + i: block q // k, slot q % k of `blocks`.  count_dev: a
        one-element int64 CUDA tensor (frame_stream's totals[:1]) that bounds the entries, or None;
        end: append Terminate's zero-length control segment.  num_data: 16-bit tensor [nblocks]
        that receives the filled slots of every touched block; seg_length: 16-bit tensor [nblocks,
        >= k] that receives 8 + len per filled slot; stats: int32 [2], packed and rejected counts
        are added (zero it first)."""
        self._need()
        b = _batch_struct(blocks, None, False)
        count = seg_start.numel()
        for t, size, what in ((seg_start, 8, "seg_start"), (seg_len, 2, "seg_len"), (seg_msg_start, 2, "seg_msg_start")):
            if t.element_size() != size or t.numel() != count or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) tensor of {count} elements of {size} bytes")
        if data.element_size() != 1 or not data.is_cuda or not data.is_contiguous():
            raise ValueError("data must be a contiguous uint8 CUDA (HIP) tensor")
        lstride = 0
        if seg_length is not None:
            if seg_length.dim() != 2 or seg_length.element_size() != 2 or seg_length.shape[0] != blocks.shape[0]:
                raise ValueError("seg_length must be a 16-bit tensor [nblocks, length_stride]")
            lstride = seg_length.shape[1]
        if num_data is not None and (num_data.element_size() != 2 or num_data.numel() < blocks.shape[0]):
            raise ValueError("num_data must be a 16-bit tensor [nblocks]")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 2):
            raise ValueError("stats must hold two 32-bit counters")
        if count_dev is not None and (count_dev.element_size() != 8 or count_dev.numel() < 1 or not count_dev.is_cuda):
            raise ValueError("count_dev must be a 64-bit CUDA (HIP) tensor")
        seg = N.StreamSegments()
        seg.bytes = data.data_ptr() if data.numel() else None
        seg.stream_bytes = data.numel()
        seg.seg_start, seg.seg_len, seg.seg_msg_start = seg_start.data_ptr(), seg_len.data_ptr(), seg_msg_start.data_ptr()
        seg.count = count
        seg.count_dev = count_dev.data_ptr() if count_dev is not None else None
        S = self.vector_size - 8 if segment_size is None else segment_size
        N.check(N.lib().nfec_stream_pack(self._h, ctypes.byref(seg), S, first_slot, write_offset & 0xFFFFFFFF,
                                         N.NFEC_STREAM_END if end else 0, ctypes.byref(b),
                                         _tensor_ptr(num_data, "num_data"), _tensor_ptr(seg_length, "seg_length"), lstride,
                                         _tensor_ptr(stats, "stats"), _stream_handle(stream)), "nfec_stream_pack")

    def unpack_stream(self, blocks, window, base_offset=0, received=None, status=None, segment_size=None, offsets=None,
                      lengths=None, msg_starts=None, stats=None, stream=None):
        """Deliver the stream segments in the source slots of a device batch to their bytes of
        `window` (uint8 CUDA tensor, any alignment; its element 0 is stream offset base_offset):
        nfec_stream_unpack.  A slot is selected as write_object selects (received / status); its
        header says where its bytes go.  Control segments (length 0) and segments whose header asks
        for more than segment_size bytes or for bytes outside the window are counted, not copied.
        offsets (32-bit), lengths and msg_starts (16-bit), each [nblocks, >= k] or None, receive
        the header fields per slot (lengths: 0xFFFF where the slot was not selected); stats: int32
        [4], delivered / not selected / control / invalid counts are added (zero it first)."""
        self._need()
        b = _batch_struct(blocks, None, False)
        if window.element_size() != 1 or not window.is_cuda or not window.is_contiguous():
            raise ValueError("window must be a contiguous uint8 CUDA (HIP) tensor")
        if received is not None:
            _mask_check(received, blocks.shape[0])
        if status is not None and (status.element_size() != 4 or status.numel() < blocks.shape[0]):
            raise ValueError("status must be a 32-bit tensor [nblocks]")
        if stats is not None and (stats.element_size() != 4 or stats.numel() < 4):
            raise ValueError("stats must hold four 32-bit counters")
        ostride = None
        for t, size, what in ((offsets, 4, "offsets"), (lengths, 2, "lengths"), (msg_starts, 2, "msg_starts")):
            if t is None:
                continue
            if t.dim() != 2 or t.element_size() != size or t.shape[0] != blocks.shape[0] or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous tensor [nblocks, out_stride] of {size}-byte elements")
            if ostride not in (None, t.shape[1]):
                raise ValueError("offsets, lengths and msg_starts must share one out_stride")
            ostride = t.shape[1]
        S = self.vector_size - 8 if segment_size is None else segment_size
        N.check(N.lib().nfec_stream_unpack(self._h, ctypes.byref(b), _tensor_ptr(received, "received"),
                                           received.shape[1] if received is not None else 0,
                                           _tensor_ptr(status, "status"), _tensor_ptr(window, "window"), window.numel(),
                                           base_offset & 0xFFFFFFFF, S, _tensor_ptr(offsets, "offsets"),
                                           _tensor_ptr(lengths, "lengths"), _tensor_ptr(msg_starts, "msg_starts"),
                                           ostride or 0, _tensor_ptr(stats, "stats"), _stream_handle(stream)),
                "nfec_stream_unpack")

    def _need(self):
        if not self._h:
            raise RuntimeError("codec not initialised (call Init)")


class _Encoder(_Codec):
    def Encode(self, segmentId, dataVector, parityVectorList, host=True):
        """NormEncoder::Encode.  host=True (the drop-in's default): nfec_encode_segment_host, the
        product on the calling CPU; host=False: the GPU round trip, nfec_encode_segment."""
        self._need()
        daddr, dkeep = _addr_ro(dataVector)
        keeps = []
        arr = (ctypes.c_void_p * self.npar)()
        for i in range(self.npar):
            a, k = _addr_rw(parityVectorList[i])
            arr[i] = a
            keeps.append(k)
        fn = "nfec_encode_segment_host" if host else "nfec_encode_segment"
        N.check(getattr(N.lib(), fn)(self._h, segmentId, daddr, arr), fn)

    def encode_blocks(self, blocks, num_data=None, accumulate=False, stream=None):
        """Parity for every block of a device batch (slots [nd, nd+m) of each block)."""
        self._need()
        b = _batch_struct(blocks, num_data, accumulate)
        N.check(N.lib().nfec_encode(self._h, ctypes.byref(b), _stream_handle(stream)), "nfec_encode")

    def encode_blocks_host(self, blocks, num_data=None, accumulate=False):
        """Same as encode_blocks for a numpy uint8 array [nblocks, slots, seg_stride] in host memory."""
        self._need()
        b = N.BlockBatch()
        b.blocks = blocks.ctypes.data
        b.block_stride = blocks.strides[0]
        b.seg_stride = blocks.strides[1]
        b.nblocks = blocks.shape[0]
        b.num_data = num_data.ctypes.data if num_data is not None else None
        b.flags = N.NFEC_ACCUMULATE if accumulate else 0
        N.check(N.lib().nfec_encode_host(self._h, ctypes.byref(b)), "nfec_encode_host")


    def encode_vectors_host(self, vectors, num_data=None, accumulate=False):
        """Batch form of CalculateBlockParity on NORM-style segment lists: vectors is a list of
        blocks, each a list of k+m (or numData_b+m) writable host buffers (numpy uint8 arrays or
        anything with a buffer) -- slots [0, numData_b) source, then m parity."""
        self._need()
        arr, keep, nd = _vector_table(vectors, self.ndata + self.npar, num_data, self.ndata)
        N.check(N.lib().nfec_encode_host_vectors(self._h, arr, len(vectors), nd,
                                                 N.NFEC_ACCUMULATE if accumulate else 0), "nfec_encode_host_vectors")


    def encode_vectors_host_async(self, vectors, num_data=None, accumulate=False):
        """encode_vectors_host queued on the codec's worker thread; returns a Request."""
        self._need()
        arr, keep, nd = _vector_table(vectors, self.ndata + self.npar, num_data, self.ndata)
        h = ctypes.c_void_p()
        N.check(N.lib().nfec_encode_host_vectors_async(self._h, arr, len(vectors), nd,
                                                       N.NFEC_ACCUMULATE if accumulate else 0, ctypes.byref(h)),
                "nfec_encode_host_vectors_async")
        return Request(h, (arr, keep, vectors, self), None)


class _Decoder(_Codec):
    def Decode(self, vectorList, numData, erasureCount, erasureLocs, host=None):
        """NormDecoder::Decode on one block.  host: None -- the drop-in's choice
        (nfec_decode_host_preferred: the host CPU for RS8 and small RS16, else the GPU);
        True / False -- force nfec_decode_vectors_host / nfec_decode_vectors."""
        self._need()
        n = numData + self.npar
        arr = (ctypes.c_void_p * n)()
        keeps = []
        for i in range(n):
            a, k = _addr_rw(vectorList[i])
            arr[i] = a
            keeps.append(k)
        locs = (ctypes.c_uint32 * max(1, erasureCount))(*list(erasureLocs)[:erasureCount])
        if host is None:
            host = N.lib().nfec_decode_host_preferred(self._h, numData, erasureCount) == 1
        if host:
            return N.check(N.lib().nfec_decode_vectors_host(self._h, arr, numData, erasureCount, locs),
                           "nfec_decode_vectors_host")
        rc = N.lib().nfec_decode_vectors(self._h, arr, numData, erasureCount, locs)
        return N.check(rc, "nfec_decode_vectors")

    def decode_blocks(self, blocks, erasure_locs, erasure_counts, num_data=None, status=None, accumulate=False,
                      stream=None):
        """Repair every block of a device batch.  erasure_locs: int16/uint16 [nblocks, stride]
        sorted slot indices; erasure_counts: int16/uint16 [nblocks]; returns int32 status
        [nblocks] (reference Decode return value per block)."""
        import torch

        self._need()
        if status is None:
            status = torch.empty(blocks.shape[0], dtype=torch.int32, device=blocks.device)
        b = _batch_struct(blocks, num_data, accumulate)
        rc = N.lib().nfec_decode(self._h, ctypes.byref(b), _tensor_ptr(erasure_locs, "erasure_locs"),
                                 erasure_locs.shape[1], _tensor_ptr(erasure_counts, "erasure_counts"),
                                 _tensor_ptr(status, "status"), _stream_handle(stream))
        N.check(rc, "nfec_decode")
        return status

    def decode_received(self, blocks, received, num_data=None, status=None, accumulate=False, stream=None):
        """decode_blocks with the erasure lists taken from the batch's reception mask
        (nfec_decode_received); returns int32 status [nblocks].  The mask is only read."""
        import torch

        self._need()
        _mask_check(received, blocks.shape[0])
        if status is None:
            status = torch.empty(blocks.shape[0], dtype=torch.int32, device=blocks.device)
        b = _batch_struct(blocks, num_data, accumulate)
        rc = N.lib().nfec_decode_received(self._h, ctypes.byref(b), _tensor_ptr(received, "received"),
                                          received.shape[1], _tensor_ptr(status, "status"), _stream_handle(stream))
        N.check(rc, "nfec_decode_received")
        return status

    def decode_blocks_host(self, blocks, erasure_locs, erasure_counts, num_data=None, accumulate=False):
        import numpy as np

        self._need()
        status = np.zeros(blocks.shape[0], np.int32)
        b = N.BlockBatch()
        b.blocks = blocks.ctypes.data
        b.block_stride = blocks.strides[0]
        b.seg_stride = blocks.strides[1]
        b.nblocks = blocks.shape[0]
        b.num_data = num_data.ctypes.data if num_data is not None else None
        b.flags = N.NFEC_ACCUMULATE if accumulate else 0
        N.check(N.lib().nfec_decode_host(self._h, ctypes.byref(b), erasure_locs.ctypes.data, erasure_locs.shape[1],
                                         erasure_counts.ctypes.data, status.ctypes.data), "nfec_decode_host")
        return status


    def decode_vectors_host_async(self, vectors, erasure_locs, erasure_counts, num_data=None, accumulate=False):
        """decode_vectors_host queued on the codec's worker thread: returns a Request at once
        (the receiver keeps going; Request.wait() gives the status array)."""
        import numpy as np

        self._need()
        arr, keep, nd = _vector_table(vectors, self.ndata + self.npar, num_data, self.ndata)
        locs = np.ascontiguousarray(erasure_locs, dtype=np.uint16)
        counts = np.ascontiguousarray(erasure_counts, dtype=np.uint16)
        status = np.zeros(len(vectors), np.int32)
        h = ctypes.c_void_p()
        N.check(N.lib().nfec_decode_host_vectors_async(self._h, arr, len(vectors), nd, locs.ctypes.data, locs.shape[1],
                                                       counts.ctypes.data, status.ctypes.data,
                                                       N.NFEC_ACCUMULATE if accumulate else 0, ctypes.byref(h)),
                "nfec_decode_host_vectors_async")
        return Request(h, (arr, keep, locs, counts, vectors, self), status)

    def decode_vectors_host(self, vectors, erasure_locs, erasure_counts, num_data=None, accumulate=False):
        """Receiver repair of many blocks given as NORM-style segment lists (None allowed for
        missing parity).  erasure_locs: uint16 [nblocks, stride]; erasure_counts: uint16
        [nblocks].  Returns int32 status [nblocks]."""
        import numpy as np

        self._need()
        arr, keep, nd = _vector_table(vectors, self.ndata + self.npar, num_data, self.ndata)
        locs = np.ascontiguousarray(erasure_locs, dtype=np.uint16)
        counts = np.ascontiguousarray(erasure_counts, dtype=np.uint16)
        status = np.zeros(len(vectors), np.int32)
        N.check(N.lib().nfec_decode_host_vectors(self._h, arr, len(vectors), nd, locs.ctypes.data, locs.shape[1],
                                                 counts.ctypes.data, status.ctypes.data,
                                                 N.NFEC_ACCUMULATE if accumulate else 0), "nfec_decode_host_vectors")
        return status


class Request:
    """An asynchronous segment-list batch (nfec_*_host_vectors_async).  Keeps the caller's
    buffers alive until completion; test() polls, wait() blocks and returns the status array
    (decode) or None (encode), raising NfecError if the call failed."""

    def __init__(self, handle, keep, status):
        self._h, self._keep, self._status = handle, keep, status

    def test(self):
        if not self._h:
            return True
        return N.check(N.lib().nfec_request_test(self._h), "nfec_request_test") == 1

    def wait(self):
        if self._h:
            h, self._h = self._h, None
            N.check(N.lib().nfec_request_wait(h), "nfec_request_wait")
            self._keep = None
        return self._status

    def __del__(self):
        try:
            self.wait()
        except Exception:
            pass


def _vector_table(vectors, n, num_data, k):
    """(void*[nblocks * n] pointer table, keep-alive list, num_data pointer or None)"""
    import numpy as np

    arr = (ctypes.c_void_p * (len(vectors) * n))()
    keep = []
    for b, blk in enumerate(vectors):
        for s, v in enumerate(blk):
            if v is None:
                continue
            a, kk = _addr_rw(v)
            arr[b * n + s] = a
            keep.append(kk)
    nd = None
    if num_data is not None:
        nd_arr = np.ascontiguousarray(num_data, dtype=np.uint16)
        keep.append(nd_arr)
        nd = nd_arr.ctypes.data
    return arr, keep, nd


class NormEncoderRS8(_Encoder):
    KIND = N.NFEC_RS8


class NormDecoderRS8(_Decoder):
    KIND = N.NFEC_RS8


class NormEncoderRS16(_Encoder):
    KIND = N.NFEC_RS16


class NormDecoderRS16(_Decoder):
    KIND = N.NFEC_RS16


class NormEncoderMDP(_Encoder):
    KIND = N.NFEC_MDP


class NormDecoderMDP(_Decoder):
    KIND = N.NFEC_MDP


# -- receiver assembly helpers --
def _mask_check(received, nblocks):
    if received.dim() != 2 or received.element_size() != 4 or received.shape[0] != nblocks:
        raise ValueError("received must be a 32-bit tensor [nblocks, mask_stride]")


def received_mask(nblocks, k, m, device="cuda"):
    """A zeroed reception mask for nblocks blocks of k + m slots: int32 [nblocks, (k + m + 31) // 32];
    bit s % 32 of word s // 32 is set once slot s holds a received segment."""
    import torch

    return torch.zeros((nblocks, (k + m + 31) // 32), dtype=torch.int32, device=device)


def erasures_from_received_host(k, m, received, num_data=None, stride=None):
    """nfec_rx_erasures_host: erasure lists from reception masks in host memory (no GPU).  received:
    NumPy 32-bit array [nblocks, mask_stride]; returns (locs uint16 [nblocks, stride], counts uint16
    [nblocks]); stride defaults to m."""
    import numpy as np

    mask = np.ascontiguousarray(received).view(np.uint32)
    if mask.ndim != 2:
        raise ValueError("received must be a 32-bit array [nblocks, mask_stride]")
    nb = mask.shape[0]
    stride = m if stride is None else stride
    locs = np.zeros((nb, stride), np.uint16)
    counts = np.zeros(nb, np.uint16)
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    N.check(N.lib().nfec_rx_erasures_host(k, m, mask.ctypes.data, mask.shape[1], None if nd is None else nd.ctypes.data,
                                          nb, locs.ctypes.data, stride, counts.ctypes.data), "nfec_rx_erasures_host")
    return locs, counts


def rx_parse_host(fec_id, fec_m, first_block_id, wire, offsets, length):
    """nfec_rx_parse_host: what ingest_messages reads in front of each payload, on host arrays (no
    GPU).  wire: NumPy uint8 array, the wire buffer; offsets 64-bit / length 16-bit arrays, one entry
    per message.  Returns (block_index uint32, symbol_id uint16, block_len uint16): the block
    relative to first_block_id inside the ID's block field, the slot, and fec_id 129's block length
    (0 for the other forms); all ones for a message that does not lie inside the buffer."""
    import numpy as np

    wire = np.ascontiguousarray(wire).view(np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    ln = np.ascontiguousarray(length, dtype=np.uint16).reshape(-1)
    if off.size != ln.size:
        raise ValueError("offsets and length must hold one entry per message")
    block_index = np.zeros(off.size, np.uint32)
    symbol_id = np.zeros(off.size, np.uint16)
    block_len = np.zeros(off.size, np.uint16)
    N.check(N.lib().nfec_rx_parse_host(fec_id, fec_m, first_block_id & 0xFFFFFFFF, wire.ctypes.data, wire.size,
                                       off.ctypes.data, ln.ctypes.data, off.size, block_index.ctypes.data,
                                       symbol_id.ctypes.data, block_len.ctypes.data), "nfec_rx_parse_host")
    return block_index, symbol_id, block_len


def data_header(source_id, instance_id, object_id, fec_id=5, fec_m=8, first_sequence=0, grtt=0, backoff=0, gsize=0,
                flags=0, fti=None):
    """nfec_data_header: the fields the NORM_DATA messages of one emit_data_messages call share.
    fti: the FTI extension's bytes as nfec_fti_write / wire.fti_write gives them (12 for fec_id 5, 16
    for 2 and 129), attached to every message, or None."""
    h = N.DataHeader()
    h.source_id, h.instance_id, h.first_sequence = source_id & 0xFFFFFFFF, instance_id & 0xFFFF, first_sequence & 0xFFFF
    h.grtt, h.backoff, h.gsize, h.flags = grtt, backoff, gsize, flags
    h.fec_id, h.fec_m, h.object_id = fec_id, fec_m, object_id & 0xFFFF
    ext = bytes(fti) if fti is not None else b""
    if len(ext) > 16:
        raise ValueError("an FTI extension has 12 or 16 bytes")
    for j, v in enumerate(ext):
        h.ext[j] = v
    h.ext_bytes = len(ext)
    return h


def data_filter(source_id, instance_id, object_id, fec_id=5, fec_m=8):
    """nfec_data_filter: the sender, code and object ingest_datagrams / rx_parse_data_host take."""
    f = N.DataFilter()
    f.source_id, f.instance_id = source_id & 0xFFFFFFFF, instance_id & 0xFFFF
    f.fec_id, f.fec_m, f.object_id = fec_id, fec_m, object_id & 0xFFFF
    return f


def data_header_bytes(fec_id, ext_bytes=0):
    """nfec_data_header_bytes: a NORM_DATA header's length, the gap to give list_pending."""
    return N.check(N.lib().nfec_data_header_bytes(fec_id, ext_bytes), "nfec_data_header_bytes")


def data_header_write_host(header, i, block_id, symbol, block_len=0):
    """nfec_data_header_write_host: the header of message i of a call, as bytes."""
    out = (ctypes.c_uint8 * 40)()
    n = N.check(N.lib().nfec_data_header_write_host(ctypes.byref(header), i & 0xFFFFFFFF, block_id & 0xFFFFFFFF, symbol,
                                                    block_len, out, 40), "nfec_data_header_write_host")
    return bytes(out[:n])


def rx_parse_data_host(filter, first_block_id, wire, offsets, length):
    """nfec_rx_parse_data_host: what ingest_datagrams reads out of each datagram, on host arrays (no
    GPU): (class uint8, sequence uint16, block_index uint32, symbol_id uint16, block_len uint16,
    payload_offset uint64, payload_length uint16, fti_index).  wire: uint8 array; offsets uint64 /
    length uint16: each datagram's start and length.  A datagram past the filter has class
    NFEC_DGRAM_PARSED; fti_index is None when no such datagram carries an FTI.  sequence is 0 where
    the datagram is unreadable."""
    import numpy as np

    wire = np.ascontiguousarray(wire, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    length = np.ascontiguousarray(length, np.uint16)
    n = offsets.size
    cls, seq = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    blk, sym, blen = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    poff, plen = np.zeros(n, np.uint64), np.zeros(n, np.uint16)
    fti = ctypes.c_uint64(0)
    N.check(N.lib().nfec_rx_parse_data_host(ctypes.byref(filter), first_block_id & 0xFFFFFFFF, wire.ctypes.data,
                                            wire.size, offsets.ctypes.data, length.ctypes.data, n, cls.ctypes.data,
                                            seq.ctypes.data, blk.ctypes.data, sym.ctypes.data, blen.ctypes.data,
                                            poff.ctypes.data, plen.ctypes.data, ctypes.addressof(fti)),
            "nfec_rx_parse_data_host")
    return cls, seq, blk, sym, blen, poff, plen, (None if fti.value == 0xFFFFFFFFFFFFFFFF else int(fti.value))


def rx_data_chunks_host(off, length):
    """nfec_rx_data_chunks_host: the positions of the aligned 16-byte chunks ingest_datagrams loads of
    a datagram at (off, length) before it knows its class."""
    out = (ctypes.c_uint64 * 3)()
    n = N.lib().nfec_rx_data_chunks_host(off, length, out)
    return [int(out[c]) for c in range(n)]


def _ctl_ext(h, ext):
    ext = bytes(ext) if ext is not None else b""
    if len(ext) not in (0, 12):
        raise ValueError("a CC-feedback extension has 12 bytes")
    for j, v in enumerate(ext):
        h.ext[j] = v
    h.ext_bytes = len(ext)


def nack_header(source_id, sender_id, instance_id, first_sequence=0, sequence_step=0, grtt_response=(0, 0), ext=None):
    """nfec_nack_header: the fields the NORM_NACK messages of one nack_messages call share.
    grtt_response: (seconds, microseconds); ext: the 12 bytes of a CC-feedback extension, or None.
    sequence_step 0 gives every message first_sequence, as the reference sends its NACKs."""
    h = N.NackHeader()
    h.source_id, h.sender_id, h.instance_id = source_id & 0xFFFFFFFF, sender_id & 0xFFFFFFFF, instance_id & 0xFFFF
    h.first_sequence, h.sequence_step = first_sequence & 0xFFFF, sequence_step & 0xFFFF
    h.grtt_response_sec, h.grtt_response_usec = grtt_response[0] & 0xFFFFFFFF, grtt_response[1] & 0xFFFFFFFF
    _ctl_ext(h, ext)
    return h


def adv_header(source_id, instance_id, sequence=0, grtt=0, backoff=0, gsize=0, ext=None):
    """nfec_adv_header: the header of the NORM_CMD(REPAIR_ADV) repair_adv_message writes."""
    h = N.AdvHeader()
    h.source_id, h.instance_id, h.sequence = source_id & 0xFFFFFFFF, instance_id & 0xFFFF, sequence & 0xFFFF
    h.grtt, h.backoff, h.gsize = grtt, backoff, gsize
    _ctl_ext(h, ext)
    return h


def ctl_filter(sender_id, instance_id, local_id=0, flags=0):
    """nfec_ctl_filter: whose control messages ingest_control / ctl_parse_host take.  flags:
    NFEC_CTL_ANY_INSTANCE | NFEC_CTL_TAKE_NACK (a sender's intake) | NFEC_CTL_TAKE_ADV (a receiver's)."""
    f = N.CtlFilter()
    f.sender_id, f.instance_id, f.local_id, f.flags = sender_id & 0xFFFFFFFF, instance_id & 0xFFFF, local_id & 0xFFFFFFFF, flags
    return f


def nack_header_bytes(ext_bytes=0):
    """nfec_nack_header_bytes: a NORM_NACK header's length, 24 or 36."""
    return N.check(N.lib().nfec_nack_header_bytes(ext_bytes), "nfec_nack_header_bytes")


def adv_header_bytes(ext_bytes=0):
    """nfec_adv_header_bytes: a NORM_CMD(REPAIR_ADV) header's length, 16 or 28."""
    return N.check(N.lib().nfec_adv_header_bytes(ext_bytes), "nfec_adv_header_bytes")


def nack_header_write_host(header, i):
    """nfec_nack_header_write_host: the header of message i of a call, as bytes."""
    out = (ctypes.c_uint8 * 36)()
    n = N.check(N.lib().nfec_nack_header_write_host(ctypes.byref(header), i & 0xFFFFFFFF, out, 36),
                "nfec_nack_header_write_host")
    return bytes(out[:n])


def nack_fragment_host(content, header, segment_size, fec_id=5, pitch=None, capacity=None):
    """nfec_nack_fragment_host: Codec.nack_messages on a host array (no GPU): (wire uint8 [capacity
    * pitch], msg_offsets uint64 [capacity], msg_length uint16 [capacity], totals uint64 [6]).
    capacity defaults to what the content could need."""
    import numpy as np

    content = np.ascontiguousarray(content, np.uint8)
    H = nack_header_bytes(header.ext_bytes)
    pitch = H + segment_size if pitch is None else pitch
    if capacity is None:
        capacity = content.size // 8 + 2
    wire = np.zeros(capacity * pitch, np.uint8)
    offs, lens = np.zeros(capacity, np.uint64), np.zeros(capacity, np.uint16)
    totals = np.zeros(6, np.uint64)
    N.check(N.lib().nfec_nack_fragment_host(content.ctypes.data, content.size, fec_id, segment_size, ctypes.byref(header),
                                            wire.ctypes.data, wire.size, pitch, offs.ctypes.data, lens.ctypes.data,
                                            capacity, totals.ctypes.data), "nfec_nack_fragment_host")
    return wire, offs, lens, totals


def adv_message_host(content, header, segment_size, fec_id=5):
    """nfec_adv_message_host: Codec.repair_adv_message on a host array (no GPU): (message bytes,
    totals uint64 [3])."""
    import numpy as np

    content = np.ascontiguousarray(content, np.uint8)
    wire = np.zeros(adv_header_bytes(header.ext_bytes) + segment_size, np.uint8)
    totals = np.zeros(3, np.uint64)
    n = N.check(N.lib().nfec_adv_message_host(content.ctypes.data, content.size, fec_id, segment_size,
                                              ctypes.byref(header), wire.ctypes.data, wire.size, totals.ctypes.data),
                "nfec_adv_message_host")
    return wire[:n].tobytes(), totals


def ctl_parse_host(filter, wire, offsets, length):
    """nfec_ctl_parse_host: Codec.ingest_control on host arrays (no GPU): (class uint8,
    content_offset uint64, content_length uint16, source_id uint32, grtt_response uint32 [count, 2],
    stats uint32 [9]).  wire: uint8 array; offsets uint64 / length uint16: each datagram's start and
    length."""
    import numpy as np

    wire = np.ascontiguousarray(wire, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    length = np.ascontiguousarray(length, np.uint16)
    n = offsets.size
    cls, coff, clen = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint16)
    src, grtt, stats = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32), np.zeros(9, np.uint32)
    N.check(N.lib().nfec_ctl_parse_host(ctypes.byref(filter), wire.ctypes.data, wire.size, offsets.ctypes.data,
                                        length.ctypes.data, n, cls.ctypes.data, coff.ctypes.data, clen.ctypes.data,
                                        src.ctypes.data, grtt.ctypes.data, stats.ctypes.data), "nfec_ctl_parse_host")
    return cls, coff, clen, src, grtt, stats


def repair_max_units(fec_id):
    """The largest max_units nfec_rx_repair_requests takes: 65535 / (2 * item length)."""
    return 65535 // (2 * (4 + N.lib().nfec_payload_id_length(fec_id)))


def repair_content_bound(k, m, nblocks, fec_id):
    """Bytes that hold the repair-request content of any nblocks masks: at most every other slot of
    a block (or every other block) starts a unit of two items with a header of its own."""
    item = 4 + N.lib().nfec_payload_id_length(fec_id)
    return nblocks * ((k + m + 1) // 2) * (4 + 2 * item) + 4 + 2 * item


def rx_repair_requests_host(k, m, received, num_data=None, fec_id=5, fec_m=8, object_id=0, first_block_id=0, flags=0,
                            max_units=None, capacity=None):
    """nfec_rx_repair_requests_host: the repair-request content of reception masks in host memory
    (no GPU).  received: NumPy 32-bit array [nblocks, mask_stride].  Returns (content uint8
    [capacity], block_start uint64 [nblocks + 1, 2], totals uint64 [4]) as Codec.repair_requests."""
    import numpy as np

    mask = np.ascontiguousarray(received).view(np.uint32)
    if mask.ndim != 2:
        raise ValueError("received must be a 32-bit array [nblocks, mask_stride]")
    nb = mask.shape[0]
    max_units = repair_max_units(fec_id) if max_units is None else max_units
    capacity = repair_content_bound(k, m, nb, fec_id) if capacity is None else capacity
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    content = np.zeros(capacity, np.uint8)
    block_start = np.zeros((nb + 1, 2), np.uint64)
    totals = np.zeros(4, np.uint64)
    N.check(N.lib().nfec_rx_repair_requests_host(k, m, mask.ctypes.data, mask.shape[1],
                                                 None if nd is None else nd.ctypes.data, nb, fec_id, fec_m,
                                                 object_id & 0xFFFF, first_block_id & 0xFFFFFFFF, flags, max_units,
                                                 content.ctypes.data, capacity, block_start.ctypes.data,
                                                 totals.ctypes.data), "nfec_rx_repair_requests_host")
    return content, block_start, totals


def repair_parse_host(fec_id, fec_m, content, capacity=None):
    """nfec_repair_parse_host: the units of repair-request content (NumPy uint8 array), as the sender
    reads a NACK.  Returns (flags uint8 [n], form uint8 [n], first uint32 [n, 4], last uint32 [n, 4],
    consumed): first / last = (object id, block id as on the wire, block length, symbol), n the units
    read before the parser stopped, consumed the offset it stopped at."""
    import numpy as np

    buf = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
    capacity = buf.size // 8 + 1 if capacity is None else capacity
    flags = np.zeros(capacity, np.uint8)
    form = np.zeros(capacity, np.uint8)
    first = np.zeros((capacity, 4), np.uint32)
    last = np.zeros((capacity, 4), np.uint32)
    consumed = ctypes.c_uint64(0)
    n = N.check(N.lib().nfec_repair_parse_host(fec_id, fec_m, buf.ctypes.data, buf.size, flags.ctypes.data,
                                               form.ctypes.data, first.ctypes.data, last.ctypes.data, capacity,
                                               ctypes.byref(consumed)), "nfec_repair_parse_host")
    n = min(n, capacity)
    return flags[:n], form[:n], first[:n], last[:n], consumed.value


class TxRepairState:
    """nfec_tx_repair_state: the sender's repair state of one object's batch.  repair 32-bit
    [nblocks, mask_stride], parity 16-bit [nblocks, 2] = (parity_offset, parity_count), block_repair
    32-bit [max(1, (nblocks + 31) // 32)], object 32-bit [1]: torch tensors on a device, or NumPy
    arrays for the *_host functions."""

    FIELDS = ("repair", "parity", "block_repair", "object")

    def __init__(self, repair, parity, block_repair, object):
        self.repair, self.parity, self.block_repair, self.object = repair, parity, block_repair, object

    @property
    def nblocks(self):
        return self.repair.shape[0]

    @property
    def mask_stride(self):
        return self.repair.shape[1]

    @property
    def on_host(self):
        return not hasattr(self.repair, "is_cuda")

    def arrays(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def struct(self):
        st = N.TxRepairStateStruct()
        for f in self.FIELDS:
            t = getattr(self, f)
            if self.on_host:
                if not t.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"state.{f} must be contiguous")
                setattr(st, f, t.ctypes.data)
            else:
                if not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"state.{f} must be a contiguous CUDA (HIP) tensor")
                setattr(st, f, t.data_ptr())
        return st

    def clone(self):
        return TxRepairState(*(t.copy() if self.on_host else t.clone() for t in self.arrays()))

    def to_host(self):
        """The state as NumPy arrays (uint32 / uint16), a copy."""
        import numpy as np

        if self.on_host:
            return self.clone()
        out = [t.cpu().numpy() for t in self.arrays()]
        return TxRepairState(out[0].view(np.uint32), out[1].view(np.uint16), out[2].view(np.uint32), out[3].view(np.uint32))

    def to_device(self, device="cuda"):
        import numpy as np
        import torch

        src = self.to_host()
        views = (src.repair.view(np.int32), src.parity.view(np.int16), src.block_repair.view(np.int32), src.object.view(np.int32))
        return TxRepairState(*(torch.from_numpy(v.copy()).to(device) for v in views))


def tx_repair_state(nblocks, k, m, auto_parity=0, device=None, mask_stride=None):
    """The repair state NormBlock::TxInit leaves (parity = (auto_parity, 0), everything else zero) for
    nblocks blocks of k + m slots: torch tensors on `device`, or NumPy arrays with device=None."""
    import numpy as np

    if not 0 <= auto_parity <= m:
        raise ValueError("auto_parity must lie in [0, m]")
    stride = (k + m + 31) // 32 if mask_stride is None else mask_stride
    parity = np.zeros((nblocks, 2), np.uint16)
    parity[:, 0] = auto_parity
    state = TxRepairState(np.zeros((nblocks, stride), np.uint32), parity, np.zeros(max(1, (nblocks + 31) // 32), np.uint32),
                          np.zeros(1, np.uint32))
    return state if device is None else state.to_device(device)


def _host_state(state, pending=None):
    import numpy as np

    if not state.on_host:
        raise ValueError("state must hold NumPy arrays (tx_repair_state(..., device=None))")
    want = (np.uint32, np.uint16, np.uint32, np.uint32)
    for f, dt in zip(state.FIELDS, want):
        if getattr(state, f).dtype != dt:
            raise ValueError(f"state.{f} must be {np.dtype(dt).name}")
    if pending is not None and (pending.dtype != np.uint32 or pending.ndim != 2 or pending.shape != state.repair.shape
                                or not pending.flags["C_CONTIGUOUS"]):
        raise ValueError("pending must be a contiguous uint32 array of state.repair's shape")
    return state.struct()


def tx_handle_nacks_host(k, m, state, payloads, offsets, length, num_data=None, fec_id=5, fec_m=8, object_id=0,
                         first_block_id=0, extra_parity=0, unit_capacity=None, count=None, payload_bytes=None):
    """nfec_tx_handle_nacks_host: Codec.handle_nacks on host arrays (no GPU), in place on `state`.
    payloads: NumPy uint8 array; offsets / length: one entry per message; count: what count_dev would
    hold, or None; payload_bytes: the wire buffer's size when it is not payloads.size.  Returns totals
    uint64 [6]."""
    import numpy as np

    wire = np.ascontiguousarray(payloads).view(np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(length, dtype=np.uint16)
    if off.size != ln.size:
        raise ValueError("offsets and length must hold one entry per message")
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    st = _host_state(state)
    unit_capacity = wire.size // 8 + 1 if unit_capacity is None else unit_capacity
    count_dev = None if count is None else np.array([count], np.uint64)
    msg = N.RxMessages()
    msg.payloads = wire.ctypes.data if wire.size else None
    msg.payload_bytes = wire.size if payload_bytes is None else payload_bytes
    msg.offsets, msg.length = off.ctypes.data, ln.ctypes.data
    msg.count = off.size
    msg.count_dev = None if count_dev is None else count_dev.ctypes.data
    totals = np.zeros(6, np.uint64)
    N.check(N.lib().nfec_tx_handle_nacks_host(k, m, ctypes.byref(msg), fec_id, fec_m, object_id & 0xFFFF,
                                              first_block_id & 0xFFFFFFFF, None if nd is None else nd.ctypes.data,
                                              state.nblocks, state.mask_stride, extra_parity, ctypes.byref(st),
                                              unit_capacity, totals.ctypes.data), "nfec_tx_handle_nacks_host")
    return totals


def tx_activate_repairs_host(k, m, state, pending, num_data=None, auto_parity=0):
    """nfec_tx_activate_repairs_host: Codec.activate_repairs on host arrays, in place on `state` and
    `pending` (uint32 [nblocks, mask_stride]).  Returns totals uint64 [3]."""
    import numpy as np

    st = _host_state(state, pending)
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    totals = np.zeros(3, np.uint64)
    N.check(N.lib().nfec_tx_activate_repairs_host(k, m, None if nd is None else nd.ctypes.data, state.nblocks, auto_parity,
                                                  pending.ctypes.data, state.mask_stride, ctypes.byref(st),
                                                  totals.ctypes.data), "nfec_tx_activate_repairs_host")
    return totals


def tx_end_blocks_host(k, m, state, pending, num_data=None):
    """nfec_tx_end_blocks_host: Codec.end_blocks on host arrays, in place on state.parity."""
    import numpy as np

    st = _host_state(state, pending)
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    N.check(N.lib().nfec_tx_end_blocks_host(k, m, None if nd is None else nd.ctypes.data, state.nblocks,
                                            pending.ctypes.data, state.mask_stride, ctypes.byref(st)),
            "nfec_tx_end_blocks_host")


class RxRepairState:
    """nfec_rx_repair_state: a receiver's suppression state of one object's batch.  repair 32-bit
    [nblocks, mask_stride], block_repair 32-bit [max(1, (nblocks + 31) // 32)], object 32-bit [1]:
    torch tensors on a device, or NumPy arrays for the *_host functions.  Zeroed at the start of a
    NACK cycle (zero())."""

    FIELDS = ("repair", "block_repair", "object")

    def __init__(self, repair, block_repair, object):
        self.repair, self.block_repair, self.object = repair, block_repair, object

    @property
    def nblocks(self):
        return self.repair.shape[0]

    @property
    def mask_stride(self):
        return self.repair.shape[1]

    @property
    def on_host(self):
        return not hasattr(self.repair, "is_cuda")

    def arrays(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def struct(self):
        st = N.RxRepairStateStruct()
        for f in self.FIELDS:
            t = getattr(self, f)
            if self.on_host:
                if not t.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"state.{f} must be contiguous")
                setattr(st, f, t.ctypes.data)
            else:
                if not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"state.{f} must be a contiguous CUDA (HIP) tensor")
                setattr(st, f, t.data_ptr())
        return st

    def zero(self):
        """The reset at the start of a NACK cycle (in stream order on a device)."""
        for t in self.arrays():
            if self.on_host:
                t[...] = 0
            else:
                t.zero_()

    def clone(self):
        return RxRepairState(*(t.copy() if self.on_host else t.clone() for t in self.arrays()))

    def to_host(self):
        """The state as NumPy uint32 arrays, a copy."""
        import numpy as np

        if self.on_host:
            return self.clone()
        return RxRepairState(*(t.cpu().numpy().view(np.uint32) for t in self.arrays()))

    def to_device(self, device="cuda"):
        import numpy as np
        import torch

        src = self.to_host()
        return RxRepairState(*(torch.from_numpy(t.view(np.int32).copy()).to(device) for t in src.arrays()))


def rx_repair_state(nblocks, k, m, device=None, mask_stride=None):
    """A zeroed suppression state for nblocks blocks of k + m slots: torch tensors on `device`, or
    NumPy arrays with device=None."""
    import numpy as np

    stride = (k + m + 31) // 32 if mask_stride is None else mask_stride
    state = RxRepairState(np.zeros((nblocks, stride), np.uint32), np.zeros(max(1, (nblocks + 31) // 32), np.uint32),
                          np.zeros(1, np.uint32))
    return state if device is None else state.to_device(device)


def _host_rx_state(state, received):
    import numpy as np

    if not state.on_host:
        raise ValueError("state must hold NumPy arrays (rx_repair_state(..., device=None))")
    for f in state.FIELDS:
        if getattr(state, f).dtype != np.uint32:
            raise ValueError(f"state.{f} must be uint32")
    mask = np.ascontiguousarray(received).view(np.uint32)
    if mask.ndim != 2 or mask.shape != state.repair.shape:
        raise ValueError("received must be a 32-bit array of state.repair's shape")
    return state.struct(), mask


def rx_handle_repair_content_host(k, m, state, received, payloads, offsets, length, num_data=None, fec_id=5, fec_m=8,
                                  object_id=0, first_block_id=0, count=None, payload_bytes=None):
    """nfec_rx_handle_repair_content_host: Codec.handle_repair_content on host arrays (no GPU), in
    place on `state`.  received: NumPy 32-bit array [nblocks, mask_stride], only read; payloads: NumPy
    uint8 array; offsets / length: one entry per message; count: what count_dev would hold, or None;
    payload_bytes: the wire buffer's size when it is not payloads.size.  Returns totals uint64 [6]."""
    import numpy as np

    wire = np.ascontiguousarray(payloads).view(np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(length, dtype=np.uint16)
    if off.size != ln.size:
        raise ValueError("offsets and length must hold one entry per message")
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    st, mask = _host_rx_state(state, received)
    count_dev = None if count is None else np.array([count], np.uint64)
    msg = N.RxMessages()
    msg.payloads = wire.ctypes.data if wire.size else None
    msg.payload_bytes = wire.size if payload_bytes is None else payload_bytes
    msg.offsets, msg.length = off.ctypes.data, ln.ctypes.data
    msg.count = off.size
    msg.count_dev = None if count_dev is None else count_dev.ctypes.data
    totals = np.zeros(6, np.uint64)
    N.check(N.lib().nfec_rx_handle_repair_content_host(k, m, ctypes.byref(msg), fec_id, fec_m, object_id & 0xFFFF,
                                                       first_block_id & 0xFFFFFFFF, mask.ctypes.data, state.mask_stride,
                                                       None if nd is None else nd.ctypes.data, state.nblocks,
                                                       ctypes.byref(st), totals.ctypes.data),
            "nfec_rx_handle_repair_content_host")
    return totals


def rx_repair_pending_host(k, m, state, received, num_data=None, flags=0):
    """nfec_rx_repair_pending_host: Codec.repair_pending on host arrays (no GPU).  Returns (totals
    uint64 [4], pending_blocks uint32 [(nblocks + 31) // 32])."""
    import numpy as np

    st, mask = _host_rx_state(state, received)
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    pending_blocks = np.full(max(1, (state.nblocks + 31) // 32), 0xFFFFFFFF if state.nblocks else 0, np.uint32)
    totals = np.zeros(4, np.uint64)
    N.check(N.lib().nfec_rx_repair_pending_host(k, m, mask.ctypes.data, state.mask_stride,
                                                None if nd is None else nd.ctypes.data, state.nblocks, ctypes.byref(st),
                                                flags, pending_blocks.ctypes.data, totals.ctypes.data),
            "nfec_rx_repair_pending_host")
    return totals, pending_blocks


def tx_repair_adv_host(k, m, state, num_data=None, fec_id=5, fec_m=8, object_id=0, first_block_id=0, max_units=None,
                       capacity=None):
    """nfec_tx_repair_adv_host: Codec.repair_adv on host arrays (no GPU).  state: a TxRepairState of
    NumPy arrays, only read.  Returns (content uint8 [capacity], block_start uint64 [nblocks + 1, 2],
    totals uint64 [4])."""
    import numpy as np

    st = _host_state(state)
    nb = state.nblocks
    max_units = repair_max_units(fec_id) if max_units is None else max_units
    capacity = repair_content_bound(k, m, nb, fec_id) if capacity is None else capacity
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    content = np.zeros(capacity, np.uint8)
    block_start = np.zeros((nb + 1, 2), np.uint64)
    totals = np.zeros(4, np.uint64)
    N.check(N.lib().nfec_tx_repair_adv_host(k, m, ctypes.byref(st), state.mask_stride,
                                            None if nd is None else nd.ctypes.data, nb, fec_id, fec_m, object_id & 0xFFFF,
                                            first_block_id & 0xFFFFFFFF, max_units, content.ctypes.data, capacity,
                                            block_start.ctypes.data, totals.ctypes.data), "nfec_tx_repair_adv_host")
    return content, block_start, totals


def tx_list_host(k, m, vector_size, pending, num_data=None, seg_length=None, gap=0, capacity=None):
    """nfec_tx_list_host: the transmission list of pending masks in host memory (no GPU).  pending:
    NumPy 32-bit array [nblocks, mask_stride]; seg_length: 16-bit array [nblocks, >= k] or None.
    Returns (offsets uint64, block_index uint32, symbol_id uint16, length uint16, block_start uint64
    [nblocks + 1, 2]); the four arrays hold `capacity` entries (default nblocks * (k + m)) and stay
    zero past the list's end."""
    import numpy as np

    mask = np.ascontiguousarray(pending).view(np.uint32)
    if mask.ndim != 2:
        raise ValueError("pending must be a 32-bit array [nblocks, mask_stride]")
    nb = mask.shape[0]
    capacity = nb * (k + m) if capacity is None else capacity
    nd = None if num_data is None else np.ascontiguousarray(num_data, dtype=np.uint16)
    lens, lstride = None, 0
    if seg_length is not None:
        lens = np.ascontiguousarray(seg_length).view(np.uint16)
        if lens.ndim != 2 or lens.shape[0] != nb:
            raise ValueError("seg_length must be a 16-bit array [nblocks, length_stride]")
        lstride = lens.shape[1]
    offsets = np.zeros(capacity, np.uint64)
    block_index = np.zeros(capacity, np.uint32)
    symbol_id = np.zeros(capacity, np.uint16)
    length = np.zeros(capacity, np.uint16)
    block_start = np.zeros((nb + 1, 2), np.uint64)
    N.check(N.lib().nfec_tx_list_host(k, m, vector_size, mask.ctypes.data, mask.shape[1],
                                      None if nd is None else nd.ctypes.data, nb,
                                      None if lens is None else lens.ctypes.data, lstride, gap, offsets.ctypes.data,
                                      block_index.ctypes.data, symbol_id.ctypes.data, length.ctypes.data, capacity,
                                      block_start.ctypes.data), "nfec_tx_list_host")
    return offsets, block_index, symbol_id, length, block_start


# -- object segmentation helpers (host rules, no GPU) --
def object_layout(object_size, segment_size, k):
    """nfec_object_layout_for: NormObject::Open's FEC block partition of a data object of object_size
    bytes in segments of segment_size bytes and blocks of at most k segments.  Returns the
    nfec_object_layout (fields as in include/nfec.h) that read_object / write_object take."""
    out = N.ObjectLayout()
    N.check(N.lib().nfec_object_layout_for(object_size, segment_size, k, ctypes.byref(out)), "nfec_object_layout_for")
    return out


def object_segment(layout, block, segment):
    """nfec_object_segment: (byte offset in the object, length) of a block's segment."""
    off, length = ctypes.c_uint64(), ctypes.c_uint32()
    N.check(N.lib().nfec_object_segment(ctypes.byref(layout), block, segment, ctypes.byref(off), ctypes.byref(length)),
            "nfec_object_segment")
    return off.value, length.value


def object_block_sizes(layout, first_block, nblocks):
    """nfec_object_block_sizes: NumPy uint16 [nblocks], the sizes of blocks first_block ... of the object."""
    import numpy as np

    out = np.zeros(nblocks, np.uint16)
    N.check(N.lib().nfec_object_block_sizes(ctypes.byref(layout), first_block, nblocks, out.ctypes.data),
            "nfec_object_block_sizes")
    return out


# -- stream framing (host rule, no GPU) --
class StreamState(N.StreamState):
    """nfec_stream_state.  StreamState() is a fresh stream: offset 0, the first write starts a message."""

    def __init__(self, write_offset=0, msg_start_pending=1, carry_bytes=0, carry_msg_start=0, next_slot=0):
        super().__init__(write_offset & 0xFFFFFFFF, msg_start_pending, carry_bytes, carry_msg_start, next_slot)

    def as_tuple(self):
        return (self.write_offset, self.msg_start_pending, self.carry_bytes, self.carry_msg_start, self.next_slot)

    def copy(self):
        return StreamState(*self.as_tuple())

    @classmethod
    def from_tensor(cls, t):
        """The state frame_stream left in its state_out tensor (synchronizes)."""
        s = N.StreamState.from_buffer_copy(t.cpu().numpy().tobytes())
        return cls(s.write_offset, s.msg_start_pending, s.carry_bytes, s.carry_msg_start, s.next_slot)


def stream_frame_host(segment_size, write_len, write_flags, state, capacity=None):
    """nfec_stream_frame_host: frame writes of a NORM stream into segments on host arrays (no GPU).
    write_len: 32-bit array [n]; write_flags: uint8 array [n] of NFEC_STREAM_EOM / NFEC_STREAM_FLUSH;
    state: a StreamState, advanced in place.  Returns (seg_start uint64, seg_len uint16,
    seg_msg_start uint16, totals uint64 [4]); the tables hold `capacity` entries (default: as many
    as the writes close) and stay zero past the list's end; totals = (segments, bytes consumed,
    carry bytes, carry_msg_start), the full numbers even past capacity."""
    import numpy as np

    wl = np.ascontiguousarray(write_len, dtype=np.uint32)
    wf = np.ascontiguousarray(write_flags, dtype=np.uint8)
    if wl.ndim != 1 or wf.shape != wl.shape:
        raise ValueError("write_len and write_flags must be one-dimensional and of one length")
    totals = np.zeros(4, np.uint64)
    if capacity is None:  # a counting call on a copy of the state
        probe = N.StreamState.from_buffer_copy(bytes(state))
        N.check(N.lib().nfec_stream_frame_host(segment_size, wl.ctypes.data, wf.ctypes.data, wl.size, ctypes.byref(probe),
                                               None, None, None, 0, totals.ctypes.data), "nfec_stream_frame_host")
        capacity = int(totals[0])
    seg_start = np.zeros(capacity, np.uint64)
    seg_len = np.zeros(capacity, np.uint16)
    seg_ms = np.zeros(capacity, np.uint16)
    N.check(N.lib().nfec_stream_frame_host(segment_size, wl.ctypes.data, wf.ctypes.data, wl.size, ctypes.byref(state),
                                           seg_start.ctypes.data, seg_len.ctypes.data, seg_ms.ctypes.data, capacity,
                                           totals.ctypes.data), "nfec_stream_frame_host")
    return seg_start, seg_len, seg_ms, totals


# -- synthetic workload helpers (device kernels) --
def fill_blocks(blocks, num_data, vector_size, seed, first_block=0, per_block_num_data=None, stream=None):
    b = _batch_struct(blocks, per_block_num_data, False)
    N.check(N.lib().nfec_util_fill(ctypes.byref(b), num_data, vector_size, seed, first_block, _stream_handle(stream)),
            "nfec_util_fill")


def stream_copy(dst, src, stream=None):
    """dst[:] = src through the streaming copy kernel (bench's achievable-HBM figure)."""
    if dst.numel() * dst.element_size() != src.numel() * src.element_size():
        raise ValueError("stream_copy: size mismatch")
    N.check(N.lib().nfec_util_stream_copy(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                          src.numel() * src.element_size(), _stream_handle(stream)),
            "nfec_util_stream_copy")


def make_erasures(nblocks, range_, count, seed, stride, first_block=0, device="cuda", stream=None):
    import torch

    locs = torch.zeros((nblocks, stride), dtype=torch.int16, device=device)
    counts = torch.zeros(nblocks, dtype=torch.int16, device=device)
    N.check(N.lib().nfec_util_erasures(ctypes.c_void_p(locs.data_ptr()), stride, ctypes.c_void_p(counts.data_ptr()),
                                       nblocks, range_, count, seed, first_block, _stream_handle(stream)),
            "nfec_util_erasures")
    return locs, counts


def zero_erasures(blocks, erasure_locs, erasure_counts, vector_size, stream=None):
    b = _batch_struct(blocks, None, False)
    N.check(N.lib().nfec_util_zero_slots(ctypes.byref(b), _tensor_ptr(erasure_locs, "erasure_locs"),
                                         erasure_locs.shape[1], _tensor_ptr(erasure_counts, "erasure_counts"),
                                         vector_size, _stream_handle(stream)), "nfec_util_zero_slots")
