// The symmetric pixel table's handle, shared by symtab.hip,
// which builds it, and coverage.hip, which walks it.
#pragma once

#include "table_walk.hpp"  // DeviceScope, dev_sort_u64

struct hh_symtab {
    int device = 0;
    int64_t n_bins = 0, nnz = 0, n_lower = 0;
    int32_t C = 0;
    hh::DBuf<unsigned short> chrom;  // chromosome of every bin
    hh::DBuf<long long> rpU, rpL;    // n_bins + 1 row pointers each
    hh::DBuf<int32_t> pU, pL;        // partners: bin2 of the upper entries (-1: out of range), bin1 of the lower ones
    hh::DBuf<double> cU, cL;         // counts: the table's, and the lower table's copy
    hh::DBuf<unsigned int> srcL;     // a lower entry's index in the upper table
};

namespace hh {

constexpr int kStSlotBits = 33;  // key = bin2 << 33 | index: n_bins < 2^31, nnz < 2^32

struct StTables {  // the device view of a handle
    const long long *rpL, *rpU;
    const int32_t *pL, *pU;
    const double *cL, *cU;
    const unsigned int* srcL;
    long long n_bins, nnz, n_lower;
};

inline StTables st_tables(const hh_symtab& H) {
    return StTables{H.rpL.p, H.rpU.p, H.pL.p, H.pU.p, H.cL.p, H.cU.p, H.srcL.p,
                    (long long)H.n_bins, (long long)H.nnz, (long long)H.n_lower};
}

}  // namespace hh
