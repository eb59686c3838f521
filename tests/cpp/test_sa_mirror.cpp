// The C++ mirror include/index4j/SuffixArray.hpp over libfmx.so, on the host-only paths (tests/test_suffix_array_cpu.py).
#include "index4j/SuffixArray.hpp"
#include <cstdio>
int main() {
    index4j::SuffixArray s(u"banana", -1, -1);
    s.construct();
    auto sa = s.getSuffixArray();
    auto back = index4j::SuffixArray::read(s.write(), -1);
    std::u16string b = index4j::BurrowsWheelerTransform::createBurrowsWheelerTransform(u"BANANA", -1);
    printf("%zu %d %d %d %zu %.3f\n", sa.size(), sa[0], s.hashCode(), back.hashCode(), b.size(),
           index4j::BurrowsWheelerTransform::computeRedundancyOfText(b));
    return b == std::u16string(u"ANNB\0AA", 7) ? 0 : 1;
}
