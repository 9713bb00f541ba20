#!/bin/bash
# Builds the emulation library with -fsanitize=address,undefined (build_emu.sh asan) and with -fsanitize=thread
# (build_emu.sh tsan), links trace_sink_standalone.cpp - a program with its own main, compiled with the same sanitizers -
# against each and runs it.  Nothing is preloaded.
set -e
cd "$(dirname "$0")"
stale() {
  [ ! -e "$1" ] || [ -n "$(find ../../luminair_amd/csrc emu_runtime.cpp -newer "$1" \( -name '*.hip' -o -name '*.cpp' -o -name '*.h' \))" ]
}
if stale libluminair_emu_asan.so; then ./build_emu.sh asan; fi
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    trace_sink_standalone.cpp -L. -lluminair_emu_asan -Wl,-rpath,"$PWD" -pthread -o trace_sink_standalone_asan
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 ./trace_sink_standalone_asan
if stale libluminair_emu_tsan.so; then ./build_emu.sh tsan; fi
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=thread \
    trace_sink_standalone.cpp -L. -lluminair_emu_tsan -Wl,-rpath,"$PWD" -pthread -o trace_sink_standalone_tsan
TSAN_OPTIONS=halt_on_error=1 ./trace_sink_standalone_tsan
