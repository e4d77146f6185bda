// The step planner on its own: syn_step_plan.inc is plain C++, so its choice of kernel is checked without a GPU and without the library
// (tests/test_host_logic.py::test_step_planner_table).  One query per line of stdin, one answer per line of stdout:
//   plan B V reserved m_tile ws_sync ws_xch ws_x0v x_fragment_order cus xcd8x32
//        -> SEQ | LAT by_seq | STACK tile_rows tp fuse_out out_tile | LAYERS tile_rows out_tile | ERROR text
//   grid B V -> workgroups of a k_seq launch
//   g++ -std=c++17 -I syntalker_amd/csrc tests/native/step_plan_host.cpp -o step_plan_host
#include <cstdio>
#include <cstring>

#include "syn_step_plan.inc"

int main() {
    char line[256], what[16];
    while (fgets(line, sizeof(line), stdin)) {
        int v[10] = {};
        const int n = sscanf(line, "%15s %d %d %d %d %d %d %d %d %d %d", what, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9]);
        if (n == 3 && !strcmp(what, "grid")) {
            printf("%d\n", seq_grid(v[0], v[1]));
            continue;
        }
        if (n != 11 || strcmp(what, "plan")) {
            fprintf(stderr, "bad query: %s", line);
            return 1;
        }
        const StepPlan p = plan_step({v[0], v[1], v[3], v[2], v[7], v[4] != 0, v[5] != 0, v[6] != 0, v[8], v[9] != 0});
        switch (p.path) {
            case STEP_SEQ:    printf("SEQ\n"); break;
            case STEP_LAT:    printf("LAT %d\n", (int)p.by_seq); break;
            case STEP_STACK:  printf("STACK %d %d %d %d\n", p.tile_rows, p.tp, (int)p.fuse_out, p.fuse_out ? 0 : p.out_tile); break;
            case STEP_LAYERS: printf("LAYERS %d %d\n", p.tile_rows, p.out_tile); break;
            case STEP_ERROR:  printf("ERROR %s\n", p.error); break;
        }
    }
    return 0;
}
