// Stand-alone run of the serial CPython set model (ysmr_amd/csrc/set_order.h: set_unused_order, what the device's
// cpython_unused_order runs) on the host.  Every line of the standard input is a case: "m table_cap k c1 .. ck" -- the k
// claimed columns of 0 .. m - 1, and the entries each of the model's two tables may hold.  Per case one line: the model's
// return value, then the order it gives the unclaimed columns (nothing more when it returns -1: the table would outgrow
// table_cap).  tests/test_cabi.py compares the orders with this interpreter's set(range(m)).difference(used).
#include "set_order.h"

#include <cstdio>
#include <vector>

int main()
{
    int m, cap, k;
    while (std::scanf("%d %d %d", &m, &cap, &k) == 3) {
        if (m < 0 || cap < 8 || k < 0 || k > m) return 2;
        std::vector<char> used(m, 0);
        for (int i = 0; i < k; ++i) {
            int c;
            if (std::scanf("%d", &c) != 1 || c < 0 || c >= m) return 2;
            used[c] = 1;
        }
        std::vector<int> unused, out(m), table(cap), other(cap);
        for (int c = 0; c < m; ++c)
            if (!used[c]) unused.push_back(c);
        const int n = set_unused_order(unused.data(), m, k, (int)unused.size(), out.data(), table.data(), other.data(), cap);
        std::printf("%d", n);
        for (int i = 0; i < n; ++i) std::printf(" %d", out[i]);
        std::printf("\n");
    }
    return 0;
}
