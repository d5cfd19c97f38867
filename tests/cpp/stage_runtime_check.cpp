// stage_runtime_check.cpp -- stand-alone check of the parts of csrc/stage_runtime.h that name no HIP symbol, and of
// EditEpoch in csrc/karto_graph_mirror.h (built with -fsanitize=address,undefined by
// tests/test_stage_runtime_cpu.py; g++ only: no HIP, no library).
//
//   stage_runtime_check poison [VALUE]   SLAM2D_POISON=VALUE (absent: unset) through poison_from_env
//   stage_runtime_check epoch N          the edit epoch of a context of N graphs, step by step
//   stage_runtime_check codes            the shared status codes and those of eleven public headers (the four
//                                        oldest have the first five)
// stdout: one JSON object.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "karto_graph_mirror.h"
#include "slam2d/gmapping.h"
#include "slam2d/hector.h"
#include "slam2d/karto.h"
#include "slam2d/karto_edit.h"
#include "slam2d/karto_grid.h"
#include "slam2d/karto_link.h"
#include "slam2d/karto_loop.h"
#include "slam2d/karto_process.h"
#include "slam2d/plicp.h"
#include "slam2d/spa.h"
#include "slam2d/undistort.h"
#include "stage_runtime.h"

using namespace s2d;

// what each capi file asserts for its own header
S2D_ASSERT_STATUS_CODES(KT);
S2D_ASSERT_STATUS_CODES(KG);
S2D_ASSERT_STATUS_CODES(SPA);
S2D_ASSERT_STATUS_CODES(KL);
S2D_ASSERT_STATUS_CODES(KE);
S2D_ASSERT_STATUS_CODES(KP);
S2D_ASSERT_STATUS_CODES(KD);
S2D_ASSERT_COMMON_CODES(HS);
S2D_ASSERT_COMMON_CODES(GM);
S2D_ASSERT_COMMON_CODES(PL);
S2D_ASSERT_COMMON_CODES(UD);

static int run_poison(const char *value)
{
    if (value) setenv("SLAM2D_POISON", value, 1);
    else unsetenv("SLAM2D_POISON");
    int poison = 7;  // a refusal and an unset variable leave it alone
    const char *why = poison_from_env(poison);
    printf("{\"refused\": %d, \"text\": \"%s\", \"poison\": %d}\n", why ? 1 : 0, why ? why : "", poison);
    return 0;
}

static void print_current(const char *name, const EditEpoch &e, int n, bool last = false)
{
    printf("\"%s\": [", name);
    for (int g = 0; g < n; ++g) printf("%s%d", g ? ", " : "", e.current(g) ? 1 : 0);
    printf("]%s", last ? "" : ", ");
}

static int run_epoch(int n)
{
    if (n < 2) return 2;
    EditEpoch e;
    e.synced.assign((size_t)n, 0);
    printf("{");
    print_current("fresh", e, n);
    e.bump();
    print_current("bumped", e, n);
    e.mark_current(1);
    print_current("marked", e, n);
    e.bump();
    print_current("bumped_again", e, n);
    // the unsigned epoch wraps: the graph that was current before the step is stale after it
    e.epoch = UINT_MAX;
    e.mark_current(0);
    print_current("before_wrap", e, n);
    e.bump();
    print_current("after_wrap", e, n);
    printf("\"epoch_after_wrap\": %u, \"seq\": %u}\n", e.epoch, e.seq);
    return 0;
}

static int run_codes()
{
    const int shared[6] = {S2D_OK, S2D_EINVAL, S2D_EHIP, S2D_ENOMEM, S2D_ENODEV, S2D_ERANGE};
    const struct {
        const char *name;
        int v[6];
    } all[] = {{"kt", {KT_OK, KT_EINVAL, KT_EHIP, KT_ENOMEM, KT_ENODEV, KT_ERANGE}},
               {"kg", {KG_OK, KG_EINVAL, KG_EHIP, KG_ENOMEM, KG_ENODEV, KG_ERANGE}},
               {"spa", {SPA_OK, SPA_EINVAL, SPA_EHIP, SPA_ENOMEM, SPA_ENODEV, SPA_ERANGE}},
               {"kl", {KL_OK, KL_EINVAL, KL_EHIP, KL_ENOMEM, KL_ENODEV, KL_ERANGE}},
               {"ke", {KE_OK, KE_EINVAL, KE_EHIP, KE_ENOMEM, KE_ENODEV, KE_ERANGE}},
               {"kp", {KP_OK, KP_EINVAL, KP_EHIP, KP_ENOMEM, KP_ENODEV, KP_ERANGE}},
               {"kd", {KD_OK, KD_EINVAL, KD_EHIP, KD_ENOMEM, KD_ENODEV, KD_ERANGE}}};
    printf("{\"s2d\": [%d, %d, %d, %d, %d, %d]", shared[0], shared[1], shared[2], shared[3], shared[4], shared[5]);
    for (const auto &m : all)
        printf(", \"%s\": [%d, %d, %d, %d, %d, %d]", m.name, m.v[0], m.v[1], m.v[2], m.v[3], m.v[4], m.v[5]);
    const struct {
        const char *name;
        int v[5];
    } common[] = {{"hs", {HS_OK, HS_EINVAL, HS_EHIP, HS_ENOMEM, HS_ENODEV}},
                  {"gm", {GM_OK, GM_EINVAL, GM_EHIP, GM_ENOMEM, GM_ENODEV}},
                  {"pl", {PL_OK, PL_EINVAL, PL_EHIP, PL_ENOMEM, PL_ENODEV}},
                  {"ud", {UD_OK, UD_EINVAL, UD_EHIP, UD_ENOMEM, UD_ENODEV}}};
    for (const auto &m : common)
        printf(", \"%s\": [%d, %d, %d, %d, %d]", m.name, m.v[0], m.v[1], m.v[2], m.v[3], m.v[4]);
    printf("}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "poison")) return run_poison(argc >= 3 ? argv[2] : nullptr);
    if (argc == 3 && !strcmp(argv[1], "epoch")) return run_epoch(atoi(argv[2]));
    if (argc == 2 && !strcmp(argv[1], "codes")) return run_codes();
    fprintf(stderr, "usage: stage_runtime_check poison [VALUE] | epoch N | codes\n");
    return 2;
}
