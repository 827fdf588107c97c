# The host twins of the NORM_NACK / REPAIR_ADV message calls (nfec_nack_fragment_host,
# nfec_nack_header_write_host, nfec_adv_message_host, nfec_ctl_parse_host) on the host under
# AddressSanitizer + UBSan, every content buffer and every datagram in an allocation of exactly its
# length (ctl_msg_asan.cpp; host code only: -fsanitize after -Xarch_host, as data_msg_asan.mk).  Not
# part of the Makefile's `all`:
#   make -C tests/native -f ctl_msg_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/ctl_msg_asan

asan_ctl_msg: $(OUT)

$(OUT): ctl_msg_asan.cpp $(CSRC)/ctl_msg_host.cpp $(CSRC)/ctl_msg.hpp $(CSRC)/data_msg.hpp $(CSRC)/nack_layout.hpp \
        $(CSRC)/rx_parse.hpp $(CSRC)/nfec_internal.hpp ../../include/nfec.h
	@mkdir -p _build
	$(HIPCC) -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -I../../include -o $@ \
	    ctl_msg_asan.cpp $(CSRC)/ctl_msg_host.cpp

.PHONY: asan_ctl_msg
