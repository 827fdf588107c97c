#!/usr/bin/env python3
"""Which kernels a call launches: a fixed list of small encode / decode batches, one named case
per invocation, to compare two builds of the library launch for launch.

    python3 tools/dispatch_trace.py --list
    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- \
        python3 tools/dispatch_trace.py run CASE > counters.json
    python3 tools/dispatch_trace.py join counters.json DIR     # one JSON line on stdout

`run` makes the codec, runs the case's call once on 9 blocks (rs_plan2_kernel's four-block
workgroups get a ragged last one) and prints the codec's path and tail counters.  `join` adds
the ordered (kernel name, grid size, workgroup size, LDS bytes) of every library kernel in the
trace.  NFEC_LIBRARY selects the build, as everywhere.  The path counters alone are too coarse:
"fixed" does not say whether the fused kernels or the unfused stages ran.

The host_* cases run a host-resident batch (nfec_*_host, nfec_*_host_vectors) in pipeline chunks
of 4 blocks: three chunks, one per slot, the last ragged; the 13-block case reuses a slot.
Trace them with `--kernel-trace --memory-copy-trace --output-format csv json`: `join` then also
gives the multiset of copies, [direction, bytes, how many] (the JSON output carries the sizes).

The *_by_layout cases reach the rungs that only a batch's layout selects on the product library
(the knobs that used to force them are compiled out of it): the batch is embedded in a pool at the
first block_stride the rung before refuses, with tests/batch_layouts.py, which names the bound of
each (`layout`: the id of one of its LADDERS; its block count replaces the 9).

The rx_ingest case runs encode, nfec_tx_list and nfec_tx_emit into a wire buffer and then the
receiver intake, nfec_rx_ingest, on that buffer.
"""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))  # batch_layouts

NB = 9
SHARED = 1  # NFEC_OPT_RS16_SHARED_TABLES
TMVP_OFF, TMVP_ON = 2, 4  # NFEC_OPT_RS16_TOEPLITZ_OFF / _ON

# name: (call, kind, k, m, vec, keyword options)
#   erase: "src16" 16 random source slots per block, "src+par" the same plus parity rows 0-15,
#          N that many random slots of the whole block
CASES = {
    "dec_rs8_64_32_v1400_fdec3": ("dec", "RS8", 64, 32, 1400, {}),
    "dec_rs8_64_32_v2048_fdec": ("dec", "RS8", 64, 32, 2048, {}),
    "dec_rs8_64_8": ("dec", "RS8", 64, 8, 1400, {"erase": 8}),
    "dec_rs8_64_32_parity_lost": ("dec", "RS8", 64, 32, 1400, {"erase": "src+par"}),
    "dec_rs8_64_32_v1397_tail": ("dec", "RS8", 64, 32, 1397, {}),
    "dec_rs8_64_32_shortened": ("dec", "RS8", 64, 32, 1400, {"short": True}),
    "dec_rs8_64_32_accumulate": ("dec", "RS8", 64, 32, 1400, {"acc": True}),
    "dec_rs8_20_10_v1000_rt": ("dec", "RS8", 20, 10, 1000, {"erase": 10}),
    "dec_rs8_20_10_v1003_rt_tail": ("dec", "RS8", 20, 10, 1003, {"erase": 10}),
    "dec_rs8_128_32": ("dec", "RS8", 128, 32, 1400, {"erase": 32}),
    "dec_mdp_64_32_v1400": ("dec", "MDP", 64, 32, 1400, {}),
    "dec_mdp_64_32_v1397": ("dec", "MDP", 64, 32, 1397, {}),
    "dec_rs16_32_8_v64_tower": ("dec", "RS16", 32, 8, 64, {"erase": 8}),
    "dec_rs16_32_8_shared_t3": ("dec", "RS16", 32, 8, 64, {"erase": 8, "opts": SHARED}),
    "dec_rs16_160_80_shared_big_plan": ("dec", "RS16", 160, 80, 64, {"erase": 80, "opts": SHARED}),
    # the smallest batch sub_batch splits: one block past the 65,536-block pass limit (38 MB)
    "dec_rs8_64_8_two_passes": ("dec", "RS8", 64, 8, 8, {"erase": 8, "nb": 65537}),
    "enc_rs8_64_32_v1400_d2": ("enc", "RS8", 64, 32, 1400, {}),
    "enc_rs8_64_32_shortened_q4": ("enc", "RS8", 64, 32, 1400, {"short": True}),
    "enc_rs8_64_32_accumulate": ("enc", "RS8", 64, 32, 1400, {"acc": True}),
    "enc_rs8_64_32_v1397_tail": ("enc", "RS8", 64, 32, 1397, {}),
    "enc_rs8_64_16": ("enc", "RS8", 64, 16, 1400, {}),
    "enc_rs8_20_10": ("enc", "RS8", 20, 10, 1400, {}),
    "enc_mdp_64_32": ("enc", "MDP", 64, 32, 1400, {}),
    "enc_mdp_64_32_shortened": ("enc", "MDP", 64, 32, 1400, {"short": True}),
    "enc_mdp_20_10": ("enc", "MDP", 20, 10, 1400, {}),
    "enc_rs16_512_128_split": ("enc", "RS16", 512, 128, 64, {}),
    "enc_rs16_32_8_shortened_tower": ("enc", "RS16", 32, 8, 64, {"short": True}),
    "enc_rs16_32_8_shared": ("enc", "RS16", 32, 8, 64, {"opts": SHARED}),
    # layout: the batch at the first block_stride past the named bound (tests/batch_layouts.py, LADDERS)
    "dec_rs8_64_32_rt_by_layout": ("dec", "RS8", 64, 32, 1400, {"layout": "dec-rs8-64-32-fixed"}),
    "dec_rs8_64_32_generic_by_layout": ("dec", "RS8", 64, 32, 1400, {"layout": "dec-rs8-64-32-generic-e16"}),
    "dec_rs8_128_127_big_plan_by_layout": ("dec", "RS8", 128, 127, 72,
                                           {"layout": "dec-rs8-128-127-generic-big-plan-a", "erase": 100, "short": True}),
    "dec_mdp_64_32_solve_by_layout": ("dec", "MDP", 64, 32, 1400, {"layout": "dec-mdp-64-32-v1400-solve-bs"}),
    "dec_mdp_64_32_v1397_generic_by_layout": ("dec", "MDP", 64, 32, 1397, {"layout": "dec-mdp-64-32", "erase": 20}),
    "dec_rs16_40_10_generic_by_layout": ("dec", "RS16", 40, 10, 64, {"layout": "dec-rs16-40-10-tower", "erase": 8}),
    "dec_rs16_40_10_shared_gather_by_layout": ("dec", "RS16", 40, 10, 64,
                                               {"layout": "dec-rs16-40-10-shared-stage1", "erase": 8, "opts": SHARED}),
    "enc_rs8_64_32_v24_q4_by_layout": ("enc", "RS8", 64, 32, 24, {"layout": "enc-rs8-64-32-t3"}),
    "enc_rs8_64_16_rt_by_layout": ("enc", "RS8", 64, 16, 1408, {"layout": "enc-rs8-64-16-fixed"}),
    "enc_rs8_20_10_generic_by_layout": ("enc", "RS8", 20, 10, 8, {"layout": "enc-rs8-20-10-rt"}),
    "enc_mdp_20_10_generic_by_layout": ("enc", "MDP", 20, 10, 8, {"layout": "enc-mdp-20-10-rt"}),
    "enc_rs16_40_10_bs_by_layout": ("enc", "RS16", 40, 10, 64, {"layout": "enc-rs16-40-10-bs", "opts": TMVP_OFF}),
    "enc_rs16_700_200_matmul_by_layout": ("enc", "RS16", 700, 200, 64,
                                          {"layout": "enc-rs16-700-200-matmul", "opts": TMVP_OFF}),
    "enc_rs16_32_8_shared_bs_by_layout": ("enc", "RS16", 32, 8, 64, {"layout": "enc-rs16-32-8-shared", "opts": SHARED | TMVP_OFF}),
    # host: "pinned" / "pageable" strided blocks, "vectors" segment lists; stride: seg_stride
    "host_enc_rs8_pinned": ("enc", "RS8", 64, 32, 1400, {"host": "pinned"}),
    "host_enc_rs8_pageable": ("enc", "RS8", 64, 32, 1400, {"host": "pageable"}),
    "host_dec_rs8_pinned": ("dec", "RS8", 64, 32, 1400, {"host": "pinned"}),
    "host_dec_rs8_pageable": ("dec", "RS8", 64, 32, 1400, {"host": "pageable"}),
    "host_enc_rs8_vectors": ("enc", "RS8", 64, 32, 1400, {"host": "vectors"}),
    "host_dec_rs8_vectors": ("dec", "RS8", 64, 32, 1400, {"host": "vectors"}),
    "host_dec_rs8_shortened_pinned": ("dec", "RS8", 64, 32, 1400, {"host": "pinned", "short": True}),
    "host_dec_mdp_24_8_v600_pageable": ("dec", "MDP", 24, 8, 600, {"host": "pageable", "erase": 8}),
    "host_enc_rs16_30_10_v998_pinned": ("enc", "RS16", 30, 10, 998, {"host": "pinned", "stride": 1000}),
    "host_dec_rs8_13_blocks_pinned": ("dec", "RS8", 64, 32, 1400, {"host": "pinned", "nb": 13}),
    # receiver intake: encode, list, emit, then nfec_rx_ingest of the wire buffer into a second batch
    "rx_ingest_rs8_64_32_v1400": ("ingest", "RS8", 64, 32, 1400, {}),
}


def _host_call(codec, call, how, blocks, nd, acc, locs=None, counts=None):
    """the case's call on a host copy of the device batch"""
    import numpy as np
    import torch

    t = blocks.cpu()
    arr = (t.pin_memory() if how == "pinned" else t).numpy()
    hnd = None if nd is None else nd.cpu().numpy().view(np.uint16)
    dec = () if call == "enc" else (locs.cpu().numpy().view(np.uint16), counts.cpu().numpy().view(np.uint16))
    torch.cuda.synchronize()
    os.environ["NFEC_HOST_CHUNK_BLOCKS"] = "4"
    if how == "vectors":
        segs = [[arr[b, s].copy() for s in range((codec.ndata if hnd is None else int(hnd[b])) + codec.npar)]
                for b in range(arr.shape[0])]
        fn = codec.encode_vectors_host if call == "enc" else codec.decode_vectors_host
    else:
        segs = arr
        fn = codec.encode_blocks_host if call == "enc" else codec.decode_blocks_host
    fn(segs, *dec, num_data=hnd, accumulate=acc)


def _embedded(ladder_id, k, m, vec):
    """the case's batch at the first block_stride its ladder's bound refuses: a strided view of a
    pool that holds just its extent, the slots zeroed (the pool's other bytes are never touched)"""
    import torch

    import batch_layouts as L

    c = L.LADDER_BY_ID[ladder_id]
    assert (c.k, c.m, c.vec) == (k, m, vec)
    lay = L.ladder_layouts(c)[-1][1]
    lay.check(k, m, vec)
    pool = torch.empty(lay.extent, dtype=torch.uint8, device="cuda")
    blocks = L.embed(pool, lay.lead, lay.nb, lay.slots, lay.seg_stride, lay.block_stride)
    for b in range(lay.nb):
        blocks[b].zero_()
    return blocks


def run(name):
    import torch

    import norm_amd.codec as C

    call, kind, k, m, vec, kw = CASES[name]
    nb, opts = kw.get("nb", NB), kw.get("opts", 0)
    enc = getattr(C, "NormEncoder" + kind)(options=opts)
    assert enc.Init(k, m, vec)
    if kw.get("layout"):
        blocks = _embedded(kw["layout"], k, m, vec)
        nb = blocks.shape[0]
    else:
        blocks = C.BlockLayout(k, m, vec, kw.get("stride")).empty(nb)
    how = kw.get("host")
    nd = None
    if kw.get("short"):
        nd = torch.tensor([k - (i % 3) for i in range(nb)], dtype=torch.int16, device="cuda")
    C.fill_blocks(blocks, k, vec, 7, per_block_num_data=nd)
    codec = enc
    if call == "enc" and how:
        _host_call(enc, call, how, blocks, nd, kw.get("acc", False))
    elif call == "enc":
        enc.encode_blocks(blocks, num_data=nd, accumulate=kw.get("acc", False))
    elif call == "ingest":
        enc.encode_blocks(blocks, num_data=nd)
        pending = torch.full((nb, (k + m + 31) // 32), -1, dtype=torch.int32, device="cuda")
        off, blk, sym, ln, start = enc.list_pending(pending, num_data=nd, gap=13)
        wire = torch.zeros(nb * (k + m) * (13 + vec), dtype=torch.uint8, device="cuda")
        enc.emit_segments(blocks, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=5, num_data=nd)
        enc.ingest_messages(torch.zeros_like(blocks), C.received_mask(nb, k, m), wire, off, ln, 5,
                            count_dev=start[nb, :1], num_data=nd)
    else:
        enc.encode_blocks(blocks, num_data=nd)
        codec = getattr(C, "NormDecoder" + kind)(options=opts)
        assert codec.Init(k, m, vec)
        erase = kw.get("erase", "src16")
        if isinstance(erase, int):
            rng = k - 2 + m if nd is not None else k + m
            locs, counts = C.make_erasures(nb, rng, erase, 11, m)
        else:
            g = torch.Generator().manual_seed(11)
            rows = []
            for _ in range(nb):
                src = sorted(torch.randperm(k - 2, generator=g)[:16].tolist())
                rows.append(src + (list(range(k, k + 16)) if erase == "src+par" else []))
            locs = torch.zeros((nb, m), dtype=torch.int16)
            locs[:, : len(rows[0])] = torch.tensor(rows, dtype=torch.int16)
            locs = locs.cuda()
            counts = torch.full((nb,), len(rows[0]), dtype=torch.int16, device="cuda")
        if not kw.get("acc"):
            C.zero_erasures(blocks, locs, counts, vec)
        if how:
            _host_call(codec, call, how, blocks, nd, kw.get("acc", False), locs, counts)
        else:
            codec.decode_blocks(blocks, locs, counts, num_data=nd, accumulate=kw.get("acc", False))
    torch.cuda.synchronize()
    print(json.dumps({"case": name, "encode_paths": enc.encode_paths(),
                      "decode_paths": codec.decode_paths() if call == "dec" else None,
                      "tail_batches": codec.tail_batches()}))


def join(counters, trace_dir):
    out = json.loads(open(counters).read().strip().splitlines()[-1])
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))  # submission order (two streams may overlap in time)

    def dims(r, stem):
        return [int(r[f"{stem}_{a}"]) for a in "XYZ" if f"{stem}_{a}" in r] or [int(r[stem])]

    out["kernels"] = [[r["Kernel_Name"].replace("nfec::(anonymous namespace)::", "").split("(")[0],
                       dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"])]
                      for r in rows if "nfec" in r["Kernel_Name"]]
    copies = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*results.json"), recursive=True):
        for tool in json.load(open(f))["rocprofiler-sdk-tool"]:
            names = []
            for e in tool.get("strings", {}).get("buffer_records", []):
                if e.get("kind") == "MEMORY_COPY":
                    names = e.get("operations", [])
            for r in tool.get("buffer_records", {}).get("memory_copy", []):
                op = r["operation"]
                key = (names[op] if isinstance(op, int) and op < len(names) else str(op), int(r["bytes"]))
                copies[key] = copies.get(key, 0) + 1
    if copies:
        out["copies"] = [[d, b, n] for (d, b), n in sorted(copies.items())]
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        print("\n".join(CASES))
    elif len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in CASES:
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "join":
        join(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
