// The one owner of device memory on the host side: move-only, frees in its destructor, grows by discarding.
// No HIP header: the runtime is reached through dev_alloc / dev_free, which engine.cpp defines with hipMalloc / hipFree
// (tests/dev_mem_host.cpp defines them over malloc).
#pragma once

#include <cstddef>
#include <utility>

namespace gd {

void *dev_alloc(size_t bytes);    // bytes > 0; throws when the device cannot give the memory
void dev_free(void *p) noexcept;  // p came from dev_alloc

class DevMem {
public:
    DevMem() = default;
    explicit DevMem(size_t bytes) : p_(dev_alloc(bytes)), bytes_(bytes) {}
    DevMem(DevMem &&o) noexcept { swap(o); }  // the source is left empty
    DevMem &operator=(DevMem &&o) noexcept {
        DevMem(std::move(o)).swap(*this);
        return *this;
    }
    ~DevMem() {
        if (p_) dev_free(p_);
    }
    void swap(DevMem &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
    }

    void *get() const { return p_; }
    size_t bytes() const { return bytes_; }

    // Grow-only, contents discarded: when `need` bytes do not fit, the block is returned FIRST (a rebuild never holds the
    // old and the new one together) and one of `grow_to` bytes is requested.  True when it reallocated.  When the request
    // throws the owner is empty.
    bool reserve(size_t need, size_t grow_to) {
        if (need <= bytes_) return false;
        DevMem().swap(*this);
        p_ = dev_alloc(grow_to);
        bytes_ = grow_to;
        return true;
    }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace gd
