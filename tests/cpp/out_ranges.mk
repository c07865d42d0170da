# out_ranges: the id ranges of agx_output_pack and the field ranges of agx_field_upload /
# agx_field_download (csrc/agx_out_ranges.hpp) held to the cascade they replaced, on the host
# under the address and undefined-behaviour sanitizers (tests/test_out_ranges_host.py builds
# and runs it: make -C tests/cpp -f out_ranges.mk)
ROOT := $(abspath ../..)
CXX ?= g++
SANFLAGS ?= -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall
out_ranges: out_ranges.cpp $(ROOT)/aither_amd/csrc/agx_out_ranges.hpp $(ROOT)/include/aither_gfx950.h
	$(CXX) $(SANFLAGS) -o $@ out_ranges.cpp
clean:
	rm -f out_ranges
.PHONY: clean
