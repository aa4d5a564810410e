// State that holds for the length of a call: set now, put back when the scope ends, on a throw as on a return.
#pragma once
#include <utility>

namespace ieache {

template <class T>
class ScopedSet {
public:
    ScopedSet(T& at, T value) : at_(at), before_(std::move(at)) { at_ = std::move(value); }
    ~ScopedSet() { at_ = std::move(before_); }
    ScopedSet(const ScopedSet&) = delete;
    ScopedSet& operator=(const ScopedSet&) = delete;

private:
    T& at_;
    T before_;
};

}  // namespace ieache
