// Stand-alone check that a change to the lowering or to pack_weights moved nothing: for each serialized plan file given it deserializes the network, lowers it,
// packs the weights and prints the lowered plan's describe_json(), every convolution-like op's offsets into the weight blob (members of a grouped launch
// included) and a 64-bit FNV-1a of the blob.  Two builds agree when their outputs are byte-identical.  No GPU is used: all of it is host work.  Link it
// against the built libtrtx_hip.so, e.g.
//   hipcc -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Itensorrtx_amd/csrc tools/plan_pack_check.cpp \
//         -Ltensorrtx_amd/lib -Wl,--no-as-needed -ltrtx_models -ltrtx_hip -Wl,-rpath,$PWD/tensorrtx_amd/lib -o plan_pack_check
// (libtrtx_models.so registers the plugin creators that the R-CNN plans name; every other plan needs libtrtx_hip.so alone) or, to run the lowering and the packing themselves under a host sanitizer, compile it TOGETHER with tensorrtx_amd/csrc/runtime/plan_passes.cpp, pack.cpp
// and plan.cpp and add -fsanitize=address,undefined -fno-omit-frame-pointer (the definitions in the program then take precedence over the library's).
// The plan files: tests/host_plan_cases.py, build(case) for each of PLAN_CASES (the int8 case needs a GPU to calibrate).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "runtime/plan.h"

using namespace trtx;

static void print_offsets(const char* what, size_t k, size_t m, const POp& op) {
    std::printf("%s %zu.%zu %s w_off %zu b_off %zu s_off %zu dw_off %zu\n", what, k, m, op_kind_name(op.kind), op.w_off, op.b_off, op.s_off, op.dw_off);
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<uint8_t> file;
        if (FILE* f = std::fopen(argv[i], "rb")) {
            uint8_t buf[1 << 16];
            for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
            std::fclose(f);
        }
        std::string err;
        std::unique_ptr<Network> net = Network::deserialize(file.data(), file.size(), &err);
        std::printf("== %s\n", argv[i]);
        if (!net) {
            std::printf("deserialize failed: %s\n", err.c_str());
            ++bad;
            continue;
        }
        Plan plan;
        if (!lower_network(*net, &plan) || !pack_weights(*net, &plan)) {
            std::printf("lowering failed: %s\n", plan.error.c_str());
            ++bad;
            continue;
        }
        std::printf("%s\n", plan.describe_json().c_str());
        for (size_t k = 0; k < plan.ops.size(); ++k) {
            print_offsets("op", k, 0, plan.ops[k]);
            for (size_t m = 0; m < plan.ops[k].group.size(); ++m) print_offsets("member", k, m, plan.ops[k].group[m]);
        }
        uint64_t h = 0xcbf29ce484222325ull;
        for (uint8_t b : plan.weight_blob) h = (h ^ b) * 0x100000001b3ull;
        std::printf("weight_blob %zu bytes fnv1a64 %016llx\n", plan.weight_blob.size(), (unsigned long long)h);
    }
    return bad != 0;
}
