// gpu_driver.hpp -- what the device test drivers of tests/cpp (*_gpu.cpp, run by the Python tests on the MI355X box) share: the readers
// and writers of the scenario files, device memory from the HIP runtime that libsdm_hip.so has already brought into the process
// (built with g++, no HIP headers, nothing further linked), the scenario header of the crop, warp and paste drivers, and the frame
// around a driver's main.  Include it behind the driver's own API header.
#pragma once
#include "sdm_cv/core.hpp"
#include "superviseddescent/hip_backend.hpp"

#include <cstdio>
#include <dlfcn.h>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

template <class T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const size_t n = (size_t)f.tellg();
    f.seekg(0);
    std::vector<T> v(n / sizeof(T));
    f.read((char*)v.data(), (std::streamsize)n);
    return v;
}

static void write_bytes(const std::string& path, const void* p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)p, (std::streamsize)n);
}

// the rows of a float32 matrix, dense
static void write_mat(const std::string& path, const cv::Mat& m)
{
    std::ofstream f(path, std::ios::binary);
    for (int r = 0; r < m.rows; ++r) f.write((const char*)m.ptr<float>(r), (std::streamsize)m.cols * 4);
}

// Device memory of a driver: every allocation is its own hipMalloc and is freed when the object goes, also when the driver throws.
// Construct it once the device is up (driver_main's Handle).
class DeviceMemory {
public:
    DeviceMemory()
    {
        malloc_ = (int (*)(void**, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
        free_ = (int (*)(void*))dlsym(RTLD_DEFAULT, "hipFree");
        memcpy_ = (int (*)(void*, const void*, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
        if (!malloc_ || !free_ || !memcpy_) throw std::runtime_error("the HIP runtime is not loaded");
    }
    ~DeviceMemory()
    {
        for (void* d : allocations_) free_(d);
    }
    DeviceMemory(const DeviceMemory&) = delete;
    DeviceMemory& operator=(const DeviceMemory&) = delete;

    uint8_t* alloc(size_t bytes)
    {
        void* d = nullptr;
        if (malloc_(&d, bytes) != 0) throw std::runtime_error("hipMalloc failed");
        allocations_.push_back(d);
        return (uint8_t*)d;
    }
    // `bytes` of src, `shift` bytes into an allocation of their own (shift: a frame's deliberate misalignment)
    uint8_t* upload(const void* src, size_t bytes, size_t shift = 0)
    {
        uint8_t* d = alloc(bytes + shift) + shift;
        if (memcpy_(d, src, bytes, 1 /* host to device */) != 0) throw std::runtime_error("hipMemcpy failed");
        return d;
    }
    void download(void* dst, const void* src_dev, size_t bytes)
    {
        if (memcpy_(dst, src_dev, bytes, 2 /* device to host */) != 0) throw std::runtime_error("hipMemcpy failed");
    }

private:
    int (*malloc_)(void**, size_t) = nullptr;
    int (*free_)(void*) = nullptr;
    int (*memcpy_)(void*, const void*, size_t, int) = nullptr;
    std::vector<void*> allocations_;
};

// <dir>/meta.txt of the crop, warp and paste drivers:
//   S w h K idx_0 ... idx_{K-1}, then per frame: format W H stride bytes and `tail` further ints that only the driver knows
struct Scenario {
    int S = 0, w = 0, h = 0;                            // rows (one frame each), crop width and height
    std::vector<int> lm;                                // the K landmark indices
    std::vector<int> fmt, W, H, stride, bytes;          // per frame
    std::vector<std::vector<int>> tail;                 // per frame

    explicit Scenario(const std::string& path, int n_tail = 0)
    {
        std::ifstream meta(path);
        int K = 0;
        meta >> S >> w >> h >> K;
        if (!meta || S < 1 || K < 0) throw std::runtime_error("cannot read " + path);
        lm.resize((size_t)K);
        for (int& v : lm) meta >> v;
        fmt.resize(S); W.resize(S); H.resize(S); stride.resize(S); bytes.resize(S);
        tail.assign((size_t)S, std::vector<int>((size_t)n_tail));
        for (int s = 0; s < S; ++s) {
            meta >> fmt[s] >> W[s] >> H[s] >> stride[s] >> bytes[s];
            for (int& v : tail[s]) meta >> v;
        }
        if (!meta) throw std::runtime_error("short " + path);
    }
};

// A driver's main: the usage line, the first handle -- so the device is up before the body makes a runtime call of its own --, and
// the body's exceptions as "error: ..." with status 1.  body(dir) returns the exit status.
template <class Body>
static int driver_main(int argc, char** argv, const char* name, Body body)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", name); return 2; }
    try {
        superviseddescent::hip::Handle first(superviseddescent::hip::device());
        return body(std::string(argv[1]));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
