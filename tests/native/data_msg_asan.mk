# The host twins of the NORM_DATA message calls (nfec_data_header_write_host, nfec_rx_parse_data_host)
# and the scatter rule's header form on the host under AddressSanitizer + UBSan, every datagram in an
# allocation of exactly its length (data_msg_asan.cpp; host code only: -fsanitize after -Xarch_host,
# as tx_repair_asan.mk).  Not part of the Makefile's `all`:
#   make -C tests/native -f data_msg_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/data_msg_asan

asan_data_msg: $(OUT)

$(OUT): data_msg_asan.cpp $(CSRC)/data_msg_host.cpp $(CSRC)/wire.cpp $(CSRC)/data_msg.hpp $(CSRC)/rx_parse.hpp \
        $(CSRC)/segment_copy.hpp $(CSRC)/nfec_internal.hpp ../../include/nfec.h
	@mkdir -p _build
	$(HIPCC) -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    data_msg_asan.cpp $(CSRC)/data_msg_host.cpp $(CSRC)/wire.cpp

.PHONY: asan_data_msg
