// Forward engine, shared types: the parsed weight records, the per-shape launch plan (buffers + ops) and the loaded model.
// netplan.hip builds a Plan from the records (parse_blob, build_plan); engine.hip binds its buffers and issues it.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "bneck.h"
#include "c3k2f32.h"
#include "c3kimg.h"
#include "ctx.h"
#include "dwpw.h"
#include "f32path.h"
#include "front.h"
#include "nnops.h"
#include "pw32.h"
#include "stem.h"

namespace obb {

static constexpr int kRegMax = 16;

struct ConvRecord {
    std::string name;
    int c1, c2, k, s, g, act;
    const float *w, *b;  // into the retained host blob copy
};

struct Buf {
    int H, W, C;
    bool f32;
    bool virt = false;  // virtual concat [nearest-x2 upsample of va | vb]: never materialised, read in place by a 1x1 conv (ConvLaunch::up_c)
    int va_buf = -1, va_co = 0, va_C = 0, vb_buf = -1, vb_co = 0, vb_C = 0;
    int blk = 0;  // > 0: channel-blocked layout [C / blk][image][pixel][blk] (TensorRef::cpb); 0 = plain NHWC
    int blk32 = 0;  // fp32 mode, 8: per-image channel blocks [image][C / 8][pixel][8] (f32path.hip C32Params): written by a conv, read by 3x3 / depthwise-prologue / virtual-concat-skip launches only
    std::string name;
    int64_t off = 0;  // byte offset into the slab per image-capacity unit (resolved at allocation)
    void *p = nullptr;
    int64_t per_img() const { return (int64_t)H * W * C; }
};

struct Slice { int buf = -1, co = 0, C = 0; };

enum OpType { OP_CONV32, OP_STEM32, OP_C3K2F32, OP_PW32, OP_CONV, OP_DW, OP_POOL, OP_UP, OP_ATTN, OP_STEM, OP_SPPF, OP_BNECK, OP_C3KIMG, OP_DWPW, OP_FRONT };

struct Op {
    OpType type;
    std::string name;
    Slice in, out, res;
    int H = 0, W = 0;        // input spatial dims
    int Ho = 0, Wo = 0;      // output spatial dims
    ConvLaunch conv;         // OP_CONV
    Conv32Launch c32;        // OP_CONV32 (fp32-arithmetic mode: f32path.hip)
    Stem32Launch stem32;     // OP_STEM32 (fp32 mode: network input layer as row stripes)
    Pw32Launch pw32;         // OP_PW32 (fp32 mode: 1x1 conv with the activations read straight from global memory into the MFMA operand)
    C3k2F32Launch c3k2f;     // OP_C3K2F32 (fp32 mode: Bottleneck + closing 1x1 of a C3k2 block in one launch)
    StemLaunch stem;         // OP_STEM (network input layer as row stripes)
    FrontLaunch front;       // OP_FRONT (model.0 + model.1 + model.2.cv1 in one launch)
    BneckLaunch bneck;       // OP_BNECK (fused Bottleneck over row stripes)
    C3kImgLaunch c3kimg;     // OP_C3KIMG (inner C3k of the stride-32 level, one persistent workgroup per image)
    DwPwLaunch dwpw;         // OP_DWPW (depthwise 3x3 -> 1x1 [-> plain 1x1 to the head] over row stripes)
    double macs = 0;         // MACs of all layers of the op (an integer: sums of them are exact in any order)
    bool one_d = false;
    bool vin = false;        // OP_CONV: the input is a virtual upsample-concat buffer
    bool upacc = false;      // OP_CONV32 with vin: reads the skip member only, its accumulators start from the coarse partial product in `ini`
    Slice ini;               //   (written by the OP_PW32 launch "<name>.up" in front of it)
    const bf16_t *dw_w = nullptr;  // OP_DW (device): 16-bit [9][C]
    const float *dw_b = nullptr;
    const float *dw_w32 = nullptr;  // OP_DW in fp32 mode: fp32 [9][C]
    int act = 0;
    int N = 0, nh = 0, kd = 0, hd = 0;  // OP_ATTN
    int head_level = -1;     // >= 0: output goes to the caller's head tensor at this level
    bool emit_cmax = false;  // this launch writes the class logits of its level through a fused tail: it can emit their per-anchor maximum too
};

struct Plan {
    int h = 0, w = 0, A = 0, no = 0, no_pad = 0;
    std::vector<Buf> bufs;
    std::vector<Op> ops;
    std::map<std::string, Slice> named;
    std::vector<void *> dev_allocs;
    int lvl_off[3] = {0, 0, 0};
    int cmax_mask = 0;  // levels whose class-logit maximum is written by the forward itself (the others: k_class_max behind it)
    int cap = 0;
    void *slab = nullptr;
    int64_t bytes_per_img = 0;
    double macs_per_img = 0;
    // sub-batch chains of one round (run_round): a stream and a join event each, one fork event on the caller's stream
    static constexpr int kLanes = 4;
    hipStream_t lanes[kLanes] = {};
    hipEvent_t ev_fork = nullptr, ev_done[kLanes] = {};
    // hipGraph cache: the ~110 launches of one forward are captured once per (sub-batch size, input pointer, output pointer) and
    // replayed; a key is captured the second time it is seen (the first run is eager: it also performs one-time attribute setup)
    typedef std::tuple<int, const void *, void *, void *> GraphKey;  // (sub-batch, tiles, head, class-logit maxima or nullptr)
    std::map<GraphKey, hipGraphExec_t> graphs;
    std::map<GraphKey, int> seen;
    std::vector<GraphKey> graph_order;  // insertion order of `graphs` (eviction)
    void drop_graphs() {
        for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
        seen.clear();
        graph_order.clear();
    }
    ~Plan() {
        drop_graphs();
        for (int i = 0; i < kLanes; ++i) {
            if (lanes[i]) (void)hipStreamDestroy(lanes[i]);
            if (ev_done[i]) (void)hipEventDestroy(ev_done[i]);
        }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        for (void *p : dev_allocs) (void)hipFree(p);
        if (slab) (void)hipFree(slab);
    }
};

struct Model {
    std::vector<char> blob;
    int nc = 0, ch = 0, max_ch = 0;
    float width = 0, depth = 0;
    std::string scale;
    std::map<std::string, ConvRecord> recs;
    int nrec_blob = 0;  // records of the weight blob itself (synthesised merged records are added to `recs` while plans are built)
    std::map<std::string, std::pair<std::vector<float>, std::vector<float>>> merged;  // weights / bias of synthesised (cout-concatenated) records
    std::map<std::pair<int, int>, std::unique_ptr<Plan>> plans;
    bf16_t *lut_dev = nullptr;
    float *lut32_dev = nullptr;  // fp32 mode: (float)v / 255.0f
    bool f32 = false;  // fp32 arithmetic end to end, one kernel per layer (obb_set_option "precision" = 32)
    bool f16 = true;  // storage precision of activations/weights (obb_set_option "precision")
    // the fused forms' switches (EngineOpts in ctx.h) as they stood at obb_model_load.  "tail" = 0 turns every intermediate-swallowing
    // form off and keeps every layer observable: `hmerge` and `bneck` are stored already and-ed with it
    EngineOpts o;
    ~Model() { if (lut_dev) (void)hipFree(lut_dev); if (lut32_dev) (void)hipFree(lut32_dev); }
};

// netplan.hip
int parse_blob(obb_ctx *ctx, Model &M);            // "OBBW" v1 blob (M.blob) -> M.recs and the model's dimensions
int build_plan(obb_ctx *ctx, Model &M, Plan &P);   // the YOLO11-OBB graph at P.h x P.w as a flat list of launches; uploads the packed weights

}  // namespace obb
