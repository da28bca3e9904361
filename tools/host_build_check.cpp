// Stand-alone driver for trtx_host_build, for running the host builders under a host sanitizer on the CPU: compile it TOGETHER with
// tensorrtx_amd/host/*.cpp (so that the builders themselves are instrumented) against the built libtrtx_hip.so, e.g.
//   hipcc -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -fsanitize=address,undefined -fno-omit-frame-pointer -I/opt/rocm/include -Iinclude \
//         tools/host_build_check.cpp tensorrtx_amd/host/*.cpp -Ltensorrtx_amd/lib -ltrtx_hip -Wl,-rpath,$PWD/tensorrtx_amd/lib -o host_build_check
// and give it groups of four arguments: model, .wts path, option string, expected status.  It builds each plan, frees it, prints one line
// per call and exits non-zero when a status is not the expected one.  No GPU is used: serializing a plan is host work.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

extern "C" int32_t trtx_host_build(const char* model, const char* wts_path, const char* options, void** blob, size_t* size);
extern "C" void trtx_host_free(void* blob);

int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i + 3 < argc; i += 4) {
        void* blob = nullptr;
        size_t size = 0;
        const int32_t st = trtx_host_build(argv[i], argv[i + 1], argv[i + 2], &blob, &size);
        const int32_t want = std::atoi(argv[i + 3]);
        std::printf("%-12s %-40s status %d (expected %d) plan %zu bytes\n", argv[i], argv[i + 2], st, want, st == 0 ? size : (size_t)0);
        if (st == 0) trtx_host_free(blob);
        bad += st != want;
    }
    std::printf("%d call(s) with an unexpected status\n", bad);
    return bad != 0;
}
