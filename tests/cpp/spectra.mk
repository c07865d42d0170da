# spectra_plan: the line, bin, chunk and twiddle-index arithmetic of the spectra
# (csrc/agx_spectra_plan.hpp), the line kernel's walk replayed on the host under the address
# and undefined-behaviour sanitizers (tests/test_spectra_host.py builds and runs it:
# make -C tests/cpp -f spectra.mk)
ROOT := $(abspath ../..)
CXX ?= g++
SANFLAGS ?= -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall
spectra_plan: spectra_plan.cpp $(ROOT)/aither_amd/csrc/agx_spectra_plan.hpp
	$(CXX) $(SANFLAGS) -o $@ spectra_plan.cpp
clean:
	rm -f spectra_plan
.PHONY: clean
