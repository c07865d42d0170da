# series_ring: the ring arithmetic of the time-series record (csrc/agx_series_ring.hpp) beside
# a std::deque, under the address and undefined-behaviour sanitizers (tests/test_series_host.py
# builds and runs it: make -C tests/cpp -f series.mk)
ROOT := $(abspath ../..)
CXX ?= g++
SANFLAGS ?= -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall
series_ring: series_ring.cpp $(ROOT)/aither_amd/csrc/agx_series_ring.hpp
	$(CXX) $(SANFLAGS) -o $@ series_ring.cpp
clean:
	rm -f series_ring
.PHONY: clean
