# mresid_plan: the patches, slots, rim loads, XCD dealing and k-chunks of the matrix residual
# (csrc/agx_mresid_plan.hpp), one step of the kernel replayed on the host under the address
# and undefined-behaviour sanitizers (tests/test_mresid_plan_host.py builds and runs it:
# make -C tests/cpp -f mresid.mk)
ROOT := $(abspath ../..)
CXX ?= g++
SANFLAGS ?= -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall
mresid_plan: mresid_plan.cpp $(ROOT)/aither_amd/csrc/agx_mresid_plan.hpp
	$(CXX) $(SANFLAGS) -o $@ mresid_plan.cpp
clean:
	rm -f mresid_plan
.PHONY: clean
