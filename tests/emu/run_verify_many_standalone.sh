#!/bin/bash
# Builds the emulation library with -fsanitize=address,undefined (build_emu.sh asan), links verify_many_standalone.cpp - a
# program with its own main, compiled with the same sanitizers - against it and runs it.  Nothing is preloaded.
set -e
cd "$(dirname "$0")"
if [ ! -e libluminair_emu_asan.so ] || [ -n "$(find ../../luminair_amd/csrc emu_runtime.cpp -newer libluminair_emu_asan.so \( -name '*.hip' -o -name '*.cpp' -o -name '*.h' \))" ]; then
  ./build_emu.sh asan
fi
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    verify_many_standalone.cpp -L. -lluminair_emu_asan -Wl,-rpath,"$PWD" -pthread -o verify_many_standalone
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 ./verify_many_standalone ../golden/kat_simple/proof
