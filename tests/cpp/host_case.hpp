// host_case.hpp -- the case-file readers of the *_host.cpp programs of tests/cpp (the kernels' per-pixel code built for the host and run
// under the host sanitizers): a value, and a length-prefixed buffer in a heap block of EXACTLY its bytes.  Never pool or pad such a
// block: a load or store that leaves the buffer is reported only because nothing of the program's lies around it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>

template <class T>
static T get(std::ifstream& f)
{
    T v;
    f.read((char*)&v, sizeof(T));
    if (!f) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
    return v;
}

// int32 bytes, then the bytes
static std::unique_ptr<uint8_t[]> block(std::ifstream& f, int& bytes)
{
    bytes = get<int>(f);
    std::unique_ptr<uint8_t[]> p(new uint8_t[bytes > 0 ? bytes : 1]);
    f.read((char*)p.get(), bytes);
    if (!f) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
    return p;
}
