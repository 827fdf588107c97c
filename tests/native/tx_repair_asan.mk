# The sender's repair state on the host (nfec_tx_handle_nacks_host, nfec_tx_activate_repairs_host,
# nfec_tx_end_blocks_host) under AddressSanitizer + UBSan, every byte a call may not touch poisoned
# (tx_repair_asan.cpp; host code only: -fsanitize after -Xarch_host, as nack_walk_asan.mk).  Not part
# of the Makefile's `all`:
#   make -C tests/native -f tx_repair_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/tx_repair_asan

asan_tx_repair: $(OUT)

$(OUT): tx_repair_asan.cpp $(CSRC)/tx_repair_host.cpp $(CSRC)/repair_layout.hpp $(CSRC)/nack_layout.hpp $(CSRC)/rx_parse.hpp \
        $(CSRC)/nfec_internal.hpp ../../include/nfec.h
	@mkdir -p _build
	$(HIPCC) -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    tx_repair_asan.cpp $(CSRC)/tx_repair_host.cpp

.PHONY: asan_tx_repair
