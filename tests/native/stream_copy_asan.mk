# The per-segment walks of nfec_stream_pack / nfec_stream_unpack on the host under AddressSanitizer +
# UBSan, every byte they may not touch poisoned (stream_copy_asan.cpp; host code only: -fsanitize
# after -Xarch_host, as segment_copy_asan.mk).  Not part of the Makefile's `all`:
#   make -C tests/native -f stream_copy_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/stream_copy_asan

asan_stream: $(OUT)

$(OUT): stream_copy_asan.cpp $(CSRC)/segment_copy.hpp $(CSRC)/stream_layout.hpp $(CSRC)/object_layout.hpp
	@mkdir -p _build
	$(HIPCC) -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    stream_copy_asan.cpp

.PHONY: asan_stream
