// init_align_carve_check.cpp — stand-alone check of init_align_kernel's LDS carve (csrc/init_align_carve.h) for every frame count;
// no GPU, no HIP.  Regions ascend without overlap, each holds what the kernel puts there for LinearAlignment (n = 3 F + 4, the larger
// of the two systems), the end is the byte count of the launch and inside a CU's LDS.  Prints one line per F (tests/test_init_align_def.py
// reads the F = 32 line); exit status 1 and a line on stderr per failed assertion.
#include <cstdio>
#include "../vins-mono_amd/csrc/init_align_carve.h"

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "F = %d: %s\n", F, #cond); g_failed = 1; } } while (0)

int main() {
    for (int F = 2; F <= AL_MAX_FRAMES; ++F) {
        const AlignLds c = align_lds(F);
        const int n = AL_N_LIN(F), tri = AL_TRI(n);
        CHECK(c.acc == 0);
        CHECK(c.acc + tri <= c.fac && c.fac + tri <= c.b);
        CHECK(c.b + n <= c.x && c.x + n <= c.col && c.col + n <= c.pr);
        CHECK(c.pr + AL_PR * (F - 1) <= c.tA && c.tA + 6 * AL_TC + 6 <= c.end);
        CHECK(AL_PR >= 7 && AL_TC >= 10);
        CHECK(c.acc % 2 == 0 && c.fac % 2 == 0 && c.b % 2 == 0 && c.x % 2 == 0 && c.col % 2 == 0 && c.pr % 2 == 0 && c.tA % 2 == 0);
        CHECK((long)c.end * 8 <= AL_CU_LDS);
        CHECK(F == 2 || c.end > align_lds(F - 1).end);                 // the launch sizes by the largest F of the batch
        printf("F %d n %d acc %d fac %d b %d x %d col %d pr %d tA %d end %d bytes %ld\n", F, n, c.acc, c.fac, c.b, c.x, c.col, c.pr,
               c.tA, c.end, (long)c.end * 8);
    }
    return g_failed;
}
