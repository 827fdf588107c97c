# The tx / rx / object kernels' two copy rules on the host under AddressSanitizer + UBSan, every
# byte they may not touch poisoned (segment_copy_asan.cpp; host code only: -fsanitize after
# -Xarch_host, as the Makefile's `asan` target builds host_gf_asan).  Not part of the Makefile's
# `all`:  make -C tests/native -f segment_copy_asan.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../norm_amd/csrc
OUT := _build/segment_copy_asan

asan_copy: $(OUT)

$(OUT): segment_copy_asan.cpp $(CSRC)/segment_copy.hpp
	@mkdir -p _build
	$(HIPCC) -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I$(CSRC) -o $@ \
	    segment_copy_asan.cpp

.PHONY: asan_copy
