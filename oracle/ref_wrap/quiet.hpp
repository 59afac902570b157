// The reference's allocator prints whole matrices to std::cout on every call.  Quiet swaps in a buffer that drops everything for
// the length of a scope and puts the old one back.
#pragma once
#include <iostream>
#include <streambuf>

namespace ref_wrap {

class Quiet {
    struct Drop : std::streambuf {
        int overflow(int c) override { return traits_type::not_eof(c); }
        std::streamsize xsputn(const char *, std::streamsize n) override { return n; }
    } drop_;
    std::streambuf *old_;

public:
    Quiet() : old_(std::cout.rdbuf(&drop_)) {}
    ~Quiet() { std::cout.rdbuf(old_); }
    Quiet(const Quiet &) = delete;
    Quiet &operator=(const Quiet &) = delete;
};

}  // namespace ref_wrap
