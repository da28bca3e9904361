// One build session: what every host builder does around its graph.  It loads the weights, creates the network (implicit or explicit
// batch), hands out the block library's context, and at the end sets the builder up and serializes.  The destructor releases, in this
// order and on every path, the scalars the blocks allocated, the network, and the weight blobs, so a builder that meets a null path
// (a plugin the creator refuses, a grid an attention block cannot split) just returns.
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace trtx_host {

// What the blocks are written against: the network, the weight map, and the 1-element scale weights of the attention blocks, which
// have to stay alive until the plan is serialized.
struct Ctx {
    nvinfer1::INetworkDefinition* net;
    WeightMap& wm;
    std::vector<float*> owned;
    nvinfer1::Weights scalar(float v) {
        float* p = new float[1]{v};
        owned.push_back(p);
        return nvinfer1::Weights{nvinfer1::DataType::kFLOAT, p, 1};
    }
};

class Session {
   public:
    // explicit_batch given: an explicit-batch network, the batch is the input's first dimension; left out: implicit batch (finish sets
    // the maximum)
    Session(nvinfer1::IBuilder* builder, const std::string& wts, int explicit_batch = kImplicit)
        : wm(loadWeights(wts)),
          net(builder->createNetworkV2(explicit_batch != kImplicit ? 1U << static_cast<uint32_t>(nvinfer1::NetworkDefinitionCreationFlag::kEXPLICIT_BATCH) : 0U)),
          c{net, wm, {}},
          batch_(explicit_batch) {}
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    ~Session() {
        for (float* p : c.owned) delete[] p;
        delete net;
        freeWeights(wm);
    }

    // (B, ch, h, w) or (ch, h, w)
    nvinfer1::ITensor* input(const char* name, int h, int w, int ch = 3) {
        nvinfer1::ITensor* t = batch_ != kImplicit ? net->addInput(name, nvinfer1::DataType::kFLOAT, nvinfer1::Dims4{batch_, ch, h, w})
                                      : net->addInput(name, nvinfer1::DataType::kFLOAT, nvinfer1::Dims3{ch, h, w});
        assert(t);
        return t;
    }
    void output(nvinfer1::ITensor* t, const char* name) {
        t->setName(name);
        net->markOutput(*t);
    }
    // debugging: the plugin's inputs as outputs "head0..N-1"
    void mark_heads(const std::vector<nvinfer1::ITensor*>& dets) {
        for (size_t i = 0; i < dets.size(); ++i) output(dets[i], ("head" + std::to_string(i)).c_str());
    }
    // max_batch is read for implicit batch only
    nvinfer1::IHostMemory* finish(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, int max_batch, bool fp16,
                                  size_t workspace = 16 * (1 << 20)) {
        if (batch_ == kImplicit) builder->setMaxBatchSize(max_batch);
        config->setMaxWorkspaceSize(workspace);
        if (fp16) config->setFlag(nvinfer1::BuilderFlag::kFP16);
        return builder->buildSerializedNetwork(*net, *config);
    }

    WeightMap wm;
    nvinfer1::INetworkDefinition* const net;
    Ctx c;

   private:
    static constexpr int kImplicit = -1;
    const int batch_;
};

}  // namespace trtx_host
