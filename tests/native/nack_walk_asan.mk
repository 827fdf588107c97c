# The per-block walk of the repair requests and the parser of their content on the host under
# AddressSanitizer + UBSan, every byte they may not touch poisoned (nack_walk_asan.cpp; host code only:
# -fsanitize after -Xarch_host, as stream_copy_asan.mk).  Not part of the Makefile's `all`:
#   make -C tests/native -f nack_walk_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/nack_walk_asan

asan_nack: $(OUT)

$(OUT): nack_walk_asan.cpp $(CSRC)/nack_layout.hpp $(CSRC)/rx_parse.hpp
	@mkdir -p _build
	$(HIPCC) -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    nack_walk_asan.cpp

.PHONY: asan_nack
