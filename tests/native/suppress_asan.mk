# NACK suppression and repair advertisements on the host (nfec_rx_handle_repair_content_host,
# nfec_rx_repair_pending_host, nfec_tx_repair_adv_host) under AddressSanitizer + UBSan, every byte a
# call may not touch poisoned (suppress_asan.cpp; host code only: -fsanitize after -Xarch_host, as
# tx_repair_asan.mk).  Not part of the Makefile's `all`:
#   make -C tests/native -f suppress_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/suppress_asan

asan_suppress: $(OUT)

$(OUT): suppress_asan.cpp $(CSRC)/suppress_host.cpp $(CSRC)/nack_host.cpp $(CSRC)/tx_repair_host.cpp $(CSRC)/suppress_layout.hpp \
        $(CSRC)/repair_layout.hpp $(CSRC)/nack_layout.hpp $(CSRC)/rx_parse.hpp $(CSRC)/nfec_internal.hpp ../../include/nfec.h
	@mkdir -p _build
	$(HIPCC) -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    suppress_asan.cpp $(CSRC)/suppress_host.cpp $(CSRC)/nack_host.cpp $(CSRC)/tx_repair_host.cpp

.PHONY: asan_suppress
