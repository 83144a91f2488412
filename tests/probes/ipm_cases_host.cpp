// ipm_cases_host.cpp — the host side of the probe's controller group: the rows of ipm_cases.h through csrc/nmpc_ipm.h as the host compiler
// builds it (no contraction of a * b + c, the C library's pow).   ipm_cases_host <rows.bin> <out.bin>: rows of ipm_cases::IN doubles in,
// ipm_cases::OUT doubles per row out.
#include <stdio.h>

#include <vector>

#include "ipm_cases.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    std::vector<double> in(ipm_cases::IN), out(ipm_cases::OUT);
    while (fread(in.data(), sizeof(double), in.size(), fi) == in.size()) {
        ipm_cases::apply(in.data(), out.data());
        if (fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 2;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
