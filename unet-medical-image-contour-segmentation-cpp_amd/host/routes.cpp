// routes.cpp -- MedicalSeg::process_single_image and process_image_batch: which device call an image takes, and what goes on around it
// (reading the files, scores against ground truth, the pipelined directory mode).  Reference: src/process.cpp:123-262,
// src/main.cpp:148-164.  The facade's units: lifecycle.cpp (state, settings, log, engine, thread contexts), artefacts.cpp (the files of
// one finished image), routes.cpp; facade.h is what the first and the last share.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <future>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>

#include "../../include/medseg/mask2polygon.h"
#include "../../include/medseg/postprocess.h"
#include "../../include/medseg/preprocess.h"
#include "facade.h"
#include "json_io.h"
#include "png_io.h"

namespace fs = std::filesystem;
using medseg::Image8;

namespace MedicalSeg {

namespace {

using hr_clock = std::chrono::high_resolution_clock;
long long ms_since(hr_clock::time_point t0) { return std::chrono::duration_cast<std::chrono::milliseconds>(hr_clock::now() - t0).count(); }

// the log file, or while it is closed a stream that takes nothing
std::ostream g_nothing(nullptr);
std::ostream &log_or_nothing() { return get_log_file().is_open() ? static_cast<std::ostream &>(get_log_file()) : g_nothing; }

// text collected during a call and written to `to` in one piece when the call ends, however it ends
struct Collected { std::ostream &to; std::ostringstream text; ~Collected() { to << text.str() << std::flush; } };

// a failure of one image or one batch: on stderr and in the log
void report(std::ostream &lg, const std::string &msg)
{
    std::cerr << msg << std::endl;
    lg << msg << std::endl;
}

// process_single_image's wording for a RAW file that cannot be read or preprocessed (src/process.cpp:211-214)
template <class Read>
auto read_or_fail(Read read) -> decltype(read())
{
    try {
        return read();
    } catch (const std::exception &e) {
        std::cerr << "preprocess_raw error: " << e.what() << '\n';
        throw std::runtime_error("Preprocessing failed");
    }
}

// ---- RAW images as the RAW-in entry points take them: one plane per image feeds every input channel of the engine -- the grey -> B,G,R
// replication of cv::imread(IMREAD_COLOR) (src/mask2polygon.cpp:117); see mi_unet_infer_raw16 in include/mi_unet.h
struct RawArgs {
    RawArgs() = default;
    RawArgs(const uint16_t *samples, int w, int h) { add(samples, w, h); }      // one image
    void add(const uint16_t *samples, int w, int h)
    {
        for (int c = 0; c < in_ch; ++c) { ptrs.push_back(samples); ws.push_back(w); hs.push_back(h); }
    }
    int images() const { return (int)ptrs.size() / in_ch; }
    const int in_ch = g_cfg.in_ch;
    std::vector<const uint16_t *> ptrs;
    std::vector<int> ws, hs;
};

// ---- where a device call goes: the calling thread's context, or a group (the engine group or a lane).  Contour capacities are
// kCapPoints / kCapContours per plane.
struct Device {
    mi_unet_t *ctx = nullptr;
    mi_unet_group_t *group = nullptr;
    int segment_raw16(const RawArgs &in, uint8_t *tiles, uint8_t *masks, int32_t *xy, int32_t *start, int32_t *counts) const
    {
        return raw_call(mi_unet_segment_raw16, mi_unet_group_segment_raw16, in, tiles, masks, xy, kCapPoints, start, kCapContours, counts);
    }
    int segment_raw16_multi(const RawArgs &in, uint8_t *tiles, uint8_t *masks, int32_t *xy, int32_t *start, int32_t *counts) const
    {
        return raw_call(mi_unet_segment_raw16_multi, mi_unet_group_segment_raw16_multi, in, tiles, masks, xy, kCapPoints, start, kCapContours,
                        counts);
    }
    int infer_raw16(const RawArgs &in, uint8_t *tiles, uint8_t *labels) const
    {
        return raw_call(mi_unet_infer_raw16, mi_unet_group_infer_raw16, in, tiles, labels, (float *)nullptr);
    }
    int last_regions(mi_unet_region *regions, int32_t *counts, int cap_planes, int *planes, int *cap_contours) const
    {
        if (ctx) return mi_unet_last_regions(ctx, regions, counts, cap_planes, planes, cap_contours);
        return mi_unet_group_last_regions(group, regions, counts, cap_planes, planes, cap_contours);
    }
    template <class OnCtx, class OnGroup, class... Out>
    int raw_call(OnCtx on_ctx, OnGroup on_group, const RawArgs &in, Out... out) const
    {
        return ctx ? on_ctx(ctx, in.ptrs.data(), in.ws.data(), in.hs.data(), in.images(), out...)
                   : on_group(group, in.ptrs.data(), in.ws.data(), in.hs.data(), in.images(), out...);
    }
};

// The region report of the last segment call on `dev`, when it measured: [planes][kCapContours] records and [planes] counts; empty when
// it did not (MedicalSeg::set_measure off).  of(plane, count): the records behind a shape list of `count` contours that the device
// traced, null when the plane has none to give.
struct RegionReport {
    RegionReport() = default;
    RegionReport(const Device &dev, size_t planes)
    {
        int pl = 0, cap = 0;
        if (dev.last_regions(nullptr, nullptr, 0, &pl, &cap) != MI_UNET_OK || (size_t)pl != planes || cap != kCapContours) return;
        regions.resize(planes * (size_t)kCapContours); counts.resize(planes);
        if (dev.last_regions(regions.data(), counts.data(), pl, &pl, &cap) != MI_UNET_OK) {
            regions.clear(); counts.clear();
        }
    }
    const mi_unet_region *of(size_t plane, int count) const
    {
        return (counts.empty() || count < 0 || counts[plane] != count) ? nullptr : regions.data() + plane * (size_t)kCapContours;
    }
    std::vector<mi_unet_region> regions;
    std::vector<int32_t> counts;
};

// channel 0 of `npix` interleaved pixels with C channels: the grey artefact tile (the planes are replicas).  In place allowed.
void keep_channel0(const uint8_t *hwc, size_t npix, int C, uint8_t *grey)
{
    for (size_t p = 0; p < npix; ++p) grey[p] = hwc[p * C];
}

std::string json_number(double v)
{
    if (!std::isfinite(v)) return "null";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// ---- set_truth_dir: the final masks of one device call against <dir>/<base>_labels.raw (u8 class indices at the tile size).
// masks holds plane (k, t) -- image k, target t, any non-zero byte = foreground -- at (k * K + t) * H * W; an empty base skips the
// image.  Every plane is recoded to 0 / 1 on both sides (the mask; truth == cls_t), so that ONE mi_unet_score_labels call with
// values = { 1 } on `h` scores all targets of all images that have a usable truth file (mi_unet_score_labels_host under
// MEDSEG_HOST_POSTPROCESS=1, or without a handle).  Writes <base>_score.json per scored image.  A missing file is a log line, a file
// of the wrong size a warning; neither fails the image, and nothing here throws.  Returns one note per image -- text for the log and
// for stderr -- or nothing at all with the truth directory off.
struct TruthNote { std::string lg, err; };

std::vector<TruthNote> score_against_truth(mi_unet_t *h, const std::vector<std::string> &bases, const uint8_t *masks,
                                           const std::vector<mi_unet_target> &targets, const std::string &output_dir)
{
    std::vector<TruthNote> notes;
    const std::string dir = get_truth_dir();
    if (dir.empty()) return notes;
    notes.resize(bases.size());
    try {
        const size_t hw = (size_t)g_cfg.height * g_cfg.width, K = targets.size();
        std::vector<size_t> good;
        std::vector<uint8_t> pred, truth, buf(hw);
        for (size_t k = 0; k < bases.size(); ++k) {
            if (bases[k].empty()) continue;
            const std::string path = dir + "/" + bases[k] + "_labels.raw";
            std::error_code ec;
            const auto size = fs::file_size(path, ec);
            if (ec) {
                notes[k].lg = "Truth: no " + path + ": not scored\n";
                continue;
            }
            std::ifstream f(path, std::ios::binary);
            if (size != hw || !f.read(reinterpret_cast<char *>(buf.data()), (std::streamsize)hw)) {
                notes[k].err = "Warning: " + path + " holds " + std::to_string(size) + " bytes, a label map of the tile " + std::to_string(hw) +
                               ": not scored\n";
                notes[k].lg = notes[k].err;
                continue;
            }
            for (size_t t = 0; t < K; ++t) {
                const uint8_t *const m = masks + (k * K + t) * hw;
                const size_t at = pred.size();
                pred.resize(at + hw); truth.resize(at + hw);
                for (size_t i = 0; i < hw; ++i) {
                    pred[at + i] = m[i] ? 1 : 0;
                    truth[at + i] = buf[i] == targets[t].cls ? 1 : 0;
                }
            }
            good.push_back(k);
        }
        if (good.empty() || K == 0) return notes;
        const int one = 1, planes = (int)(good.size() * K);
        const mi_unet_score_opts opts{ 50000, 0 };
        std::vector<mi_unet_score> scores((size_t)planes);
        const int rc = (h && device_postprocess_requested())
                           ? mi_unet_score_labels(h, pred.data(), truth.data(), planes, g_cfg.height, g_cfg.width, &one, 1, &opts, scores.data(), nullptr, nullptr)
                           : mi_unet_score_labels_host(pred.data(), truth.data(), planes, g_cfg.height, g_cfg.width, &one, 1, &opts, scores.data(), nullptr, nullptr);
        for (size_t g = 0; g < good.size(); ++g) {
            TruthNote &note = notes[good[g]];
            if (rc != MI_UNET_OK) {
                note.err = note.lg = std::string("Warning: scoring failed: ") + mi_unet_last_error() + "\n";
                continue;
            }
            std::ostringstream js;
            js << "{\n  \"quantile_ppm\": " << opts.quantile_ppm << ",\n  \"targets\": [";
            for (size_t t = 0; t < K; ++t) {
                const mi_unet_score &sc = scores[g * K + t];
                mi_unet_score_metrics m{};
                (void)mi_unet_score_derive(&sc, &m);
                js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"tp\": " << sc.tp << ", \"fp\": " << sc.fp << ", \"fn\": " << sc.fn
                   << ", \"dice\": " << json_number(m.dice) << ", \"iou\": " << json_number(m.iou) << ", \"hd\": " << json_number(m.hd)
                   << ", \"hd_q\": " << json_number(m.hd_q) << ", \"assd\": " << json_number(m.assd) << ", \"rmsd\": " << json_number(m.rmsd) << "}";
            }
            js << "\n  ]\n}\n";
            const std::string out_path = output_dir + "/" + bases[good[g]] + "_score.json";
            std::ofstream o(out_path, std::ios::binary);
            o << js.str();
            o.close();
            if (!o) note.err = note.lg = "Warning: cannot write " + out_path + "\n";
            else note.lg = "Score: " + out_path + "\n";
        }
    } catch (const std::exception &e) {
        for (TruthNote &n : notes)
            if (n.lg.empty()) n.err = n.lg = std::string("Warning: scoring failed: ") + e.what() + "\n";
    }
    return notes;
}

// the scores of one device call, and their notes handed out: stderr, and the log text to `lg`
void score_and_note(mi_unet_t *h, const std::vector<std::string> &bases, const uint8_t *masks, const std::vector<mi_unet_target> &targets,
                    const std::string &output_dir, std::ostream &lg)
{
    for (const TruthNote &note : score_against_truth(h, bases, masks, targets, output_dir)) {
        std::cerr << note.err << std::flush;
        lg << note.lg << std::flush;
    }
}

const std::vector<mi_unet_target> kReferenceTarget{ { 2, 0.06f } };

// One image of the default target after the device work is done, on the routes with a host tail: write the reference's artefacts and
// run the CPU tail of the pipeline.  The last step is Mask2Polygon::process_single_mask, not write_image_artefacts: it reads the PNGs
// back from disk as the reference does and deflates the overlay, so its files and console text are its own.  With a truth
// directory the postprocessed mask is scored on `score_h` (under `score_lock` when given), the note going to `lg`.
void finish_image(const std::string &raw_path, int width, int height, const std::string &output_dir, const Image8 &tile,
                  Image8 pred_mask, bool already_postprocessed, mi_unet_t *score_h, std::mutex *score_lock, std::ostream &lg)
{
    const std::string base_name = fs::path(raw_path).stem().string();
    const std::string preprocessed_png_path = output_dir + "/" + base_name + "_normalized.png";
    const std::string size_json_path = output_dir + "/" + base_name + "_original_sizes.json";
    const std::string pred_mask_path = output_dir + "/" + base_name + "_mask.png";
    if (!Preprocess::write_preprocess_outputs(tile, raw_path, preprocessed_png_path, size_json_path, width, height))
        throw std::runtime_error("Preprocessing failed");
    if (!already_postprocessed) pred_mask = postprocess_mask(pred_mask);
    if (!medseg::write_png(pred_mask_path, mask_to_image(pred_mask), /*level0=*/true))
        throw std::runtime_error("Failed to save mask");
    if (!get_truth_dir().empty()) {
        std::unique_lock<std::mutex> lk;
        if (score_lock) lk = std::unique_lock<std::mutex>(*score_lock);
        score_and_note(score_h, { base_name }, pred_mask.data.data(), kReferenceTarget, output_dir, lg);
    }
    Mask2Polygon::process_single_mask(pred_mask_path, output_dir, size_json_path, preprocessed_png_path, base_name);
}

// ---- directory mode as a three-stage pipeline over chunks of max_batch images (all-device route):
//        read the files of chunk k+1  ||  device: chunk k (mi_unet_segment_raw16)  ||  PNG / JSON artefacts of chunk k-1
// Each stage is internally parallel over its images (a few host threads; the device call is one micro-batch); console and
// log text is collected per image and emitted in file order, chunk after chunk, by the calling thread.
// Page-locked buffers for the RAW files of directory mode (mi_unet_host_alloc): the reader threads copy page cache -> pinned,
// the engine's DMA reads them directly, and the device thread no longer pays a staging memcpy per image.  Pinning memory is
// slow (a millisecond per 6 MB), so buffers are recycled across chunks and calls and released by cleanup_resources().
class PinnedPool {
public:
    struct Buf { uint16_t *p = nullptr; size_t cap = 0; };
    Buf acquire(size_t samples)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].cap >= samples) { Buf b = free_[i]; free_.erase(free_.begin() + i); return b; }
        }
        Buf b;
        void *p = nullptr;
        if (mi_unet_host_alloc(samples * sizeof(uint16_t), &p) != MI_UNET_OK) throw std::runtime_error(std::string("pinned allocation failed: ") + mi_unet_last_error());
        b.p = static_cast<uint16_t *>(p); b.cap = samples;
        return b;
    }
    void release(Buf b)
    {
        if (!b.p) return;
        std::lock_guard<std::mutex> lk(m_);
        free_.push_back(b);
    }
    void clear()
    {
        std::lock_guard<std::mutex> lk(m_);
        for (Buf &b : free_) mi_unet_host_free(b.p);
        free_.clear();
    }

private:
    std::mutex m_;
    std::vector<Buf> free_;
};
PinnedPool g_pinned;

struct ChunkIn {
    size_t first = 0, count = 0;                       // range of the caller's lists
    std::vector<PinnedPool::Buf> raws;                 // per file of the range (p == nullptr: unreadable)
    std::vector<std::string> read_err;
    long long read_ms = 0;
};

struct ChunkOut {
    std::vector<size_t> idx;                           // files of the range that were read (offsets into the range)
    std::vector<uint8_t> tiles, labels;
    std::vector<int32_t> xy, start, cnt;
    RegionReport regions;                              // set_measure: of the m planes, else empty
    std::vector<TruthNote> truth;                      // set_truth_dir: one note per read file, else empty
    long long device_ms = 0;
};

struct ChunkText {
    std::vector<std::string> con, err, lg;             // per read file: console, stderr, log text
    int ok = 0;
    long long art_ms = 0;
};

// I/O and artefact threads of directory mode: one per image of the chunk up to MEDSEG_IO_THREADS (default 16 -- a GPU's share of a
// host, never the whole machine: an 8-GPU node runs eight of these pools)
int io_threads_for(size_t n)
{
    static const int cap = std::max(1, env_int("MEDSEG_IO_THREADS", 16));
    return (int)std::max<size_t>(1, std::min<size_t>(n, (size_t)cap));
}

ChunkIn read_chunk(const std::vector<std::string> &paths, const std::vector<int> &widths, const std::vector<int> &heights,
                   size_t first, size_t count)
{
    ChunkIn in;
    in.first = first; in.count = count;
    in.raws.resize(count); in.read_err.resize(count);
    const auto t0 = hr_clock::now();
    const int nt = io_threads_for(count);
#pragma omp parallel for schedule(dynamic) num_threads(nt)
    for (long long k = 0; k < (long long)count; ++k) {
        try {
            const Preprocess::RawView view(paths[first + k], widths[first + k], heights[first + k]);
            in.raws[k] = g_pinned.acquire(view.samples());
            std::memcpy(in.raws[k].p, view.data(), view.samples() * sizeof(uint16_t));
        } catch (const std::exception &e) {
            in.read_err[k] = std::string("Processing error: ") + e.what() + " (" + paths[first + k] + ")";
            g_pinned.release(in.raws[k]);
            in.raws[k] = PinnedPool::Buf{};
        }
    }
    in.read_ms = ms_since(t0);
    return in;
}

ChunkOut device_chunk(const ChunkIn &in, const std::vector<std::string> &paths, const std::vector<int> &widths, const std::vector<int> &heights,
                      const std::string &output_dir, mi_unet_group_t *group)
{
    ChunkOut out;
    const int C = g_cfg.in_ch;
    RawArgs raws;
    for (size_t k = 0; k < in.count; ++k)
        if (in.read_err[k].empty()) {
            out.idx.push_back(k);
            raws.add(in.raws[k].p, widths[in.first + k], heights[in.first + k]);
        }
    if (out.idx.empty()) return out;
    const size_t hw = (size_t)g_cfg.height * g_cfg.width, m = out.idx.size();
    std::vector<uint8_t> tiles_c(C > 1 ? hw * m * C : 0);
    out.tiles.resize(hw * m); out.labels.resize(hw * m);
    out.xy.resize(m * kCapPoints * 2); out.start.resize(m * (kCapContours + 1)); out.cnt.resize(m);
    const auto t0 = hr_clock::now();
    const Device dev{ nullptr, group };
    if (dev.segment_raw16(raws, C > 1 ? tiles_c.data() : out.tiles.data(), out.labels.data(), out.xy.data(), out.start.data(),
                          out.cnt.data()) != MI_UNET_OK)
        throw std::runtime_error(std::string("Inference failed: ") + mi_unet_last_error());
    out.regions = RegionReport(dev, m);
    if (!get_truth_dir().empty()) {                    // one scoring call for the chunk, on the lane's first engine
        std::vector<std::string> bases;
        for (size_t k : out.idx) bases.push_back(fs::path(paths[in.first + k]).stem().string());
        out.truth = score_against_truth(mi_unet_group_handle(group, 0), bases, out.labels.data(), kReferenceTarget, output_dir);
    }
    if (C > 1) keep_channel0(tiles_c.data(), hw * m, C, out.tiles.data());
    out.device_ms = ms_since(t0);
    return out;
}

ChunkText artefact_chunk(const ChunkIn &in, const ChunkOut &out, const std::vector<std::string> &paths, const std::vector<int> &widths,
                         const std::vector<int> &heights, const std::string &output_dir)
{
    const size_t m = out.idx.size();
    ChunkText tx;
    tx.con.resize(m); tx.err.resize(m); tx.lg.resize(m);
    std::vector<char> done(m, 0);
    const auto t0 = hr_clock::now();
    const int nt = io_threads_for(m);
#pragma omp parallel for schedule(dynamic) num_threads(nt)
    for (long long k = 0; k < (long long)m; ++k) {
        const size_t i = in.first + out.idx[k];
        std::ostringstream con, lg;
        medseg::set_png_threads(m > 1 ? 1 : 16);    // the images of a chunk are already written in parallel: no band threads inside
        try {
            const std::string base_name = fs::path(paths[i]).stem().string();
            lg << "\n=== Processing Image: " << fs::path(paths[i]).filename().string() << " ===" << std::endl;
            const Image8 tile = tile_image(out.tiles, k), vis = tile_image(out.labels, k);
            const PlaneShapes shapes{ &out.xy[k * (size_t)kCapPoints * 2], &out.start[k * (kCapContours + 1)], out.cnt[k],
                                      out.regions.of((size_t)k, out.cnt[k]) };
            ImageArtefacts a;
            a.tile = &tile; a.targets = &kReferenceTarget; a.masks = &vis; a.planes = &shapes; a.width = widths[i]; a.height = heights[i];
            a.raw_path = paths[i]; a.output_dir = output_dir; a.base_name = base_name; a.console = &con;
            write_image_artefacts(a);
            if (!out.truth.empty()) {
                lg << out.truth[k].lg;
                tx.err[k] += out.truth[k].err;
            }
            lg << "Processing completed for: " << base_name << std::endl;
            done[k] = 1;
        } catch (const std::exception &e) {
            tx.err[k] = std::string("Processing error: ") + e.what() + "\n";
            lg << "Processing error: " << e.what() << std::endl;
        }
        tx.con[k] = con.str(); tx.lg[k] = lg.str();
    }
    for (size_t k = 0; k < m; ++k) tx.ok += done[k];
    tx.art_ms = ms_since(t0);
    return tx;
}

// the all-device route of process_image_batch; returns the number of images that succeeded.
// Stages: read the files of chunk k+1 || device work of chunk k || PNG / JSON artefacts of chunk k-1.
// Two device lanes by default when the call has more than one piece (the second lane is a clone of the engine group: shared weights, own
// buffers / streams / worker threads), so that the exposed head of one piece's device call (upload + preprocess of its first images) and
// its tail (postprocess, contours, download of its last ones) run beside the other piece's network.  Round 3 measured no gain from it
// (1.77 vs 1.78 ms per image over 64 files: the file reads were the critical path then); with the reads out of the way -- MAP_POPULATE,
// host/preprocess.cpp -- same card, two rounds: 16 files 626 / 615 -> 647 / 652 images/s, 64 files 702 / 699 -> 804 / 719
// (profiles/r04_facade_chunks.txt).  MEDSEG_DEVICE_LANES=1 keeps one lane (half the activation memory).
int process_batch_pipelined(const std::vector<std::string> &paths, const std::vector<int> &widths, const std::vector<int> &heights,
                            const std::string &output_dir)
{
    std::ostream &log_file = log_or_nothing();
    mi_unet_group_t *lanes[2];
    // (a second lane only with more than one piece: see `step` below)
    const int n_lanes = device_lanes(lanes, paths.size() >= 16 && env_int("MEDSEG_DEVICE_LANES", 2) >= 2);
    // a chunk = one micro-batch on every device of the group ... unless the whole call fits into one: then it is cut into four
    // pieces (at least four images each), so that reading piece k + 1, the device work of k (two lanes: k and k + 1) and the
    // artefacts of k - 1 overlap inside a 16-file call too.  Same card, 16 files, one lane: one piece 568, two 596, four 534 images/s
    // (smaller network batches cost more than the overlap returns); two lanes: one piece 527, two 615-637, four 674
    // (profiles/r04_facade_chunks.txt; MEDSEG_PIPELINE_CHUNK overrides the piece size)
    const size_t n = paths.size(), full = (size_t)std::max(1, g_cfg.max_batch) * (size_t)std::max(1, mi_unet_group_size(lanes[0]));
    size_t step = full;
    if (n <= full) step = n_lanes == 2 ? std::max<size_t>(4, (n + 3) / 4) : std::max<size_t>(8, (n + 1) / 2);
    if (const int forced = env_int("MEDSEG_PIPELINE_CHUNK", 0); forced > 0) step = std::min<size_t>(full, (size_t)forced);
    int ok = 0;
    auto emit = [&](const ChunkIn &in, const ChunkOut &out, const ChunkText &tx) {
        for (size_t k = 0; k < tx.con.size(); ++k) {
            std::cout << tx.con[k] << std::flush;
            std::cerr << tx.err[k] << std::flush;
            log_file << tx.lg[k] << std::flush;
        }
        log_file << "Batch read time: " << in.read_ms << " ms for " << in.count << " files; Batch device time: " << out.device_ms
                     << " ms for " << out.idx.size() << " images; Batch artefact time: " << tx.art_ms << " ms" << std::endl;
        ok += tx.ok;
    };
    struct Stage { ChunkIn in; ChunkOut out; std::string dev_err; };
    struct InFlight { std::shared_ptr<Stage> st; std::future<void> done; };
    std::vector<InFlight> dev_q;                       // device work in flight, oldest first, at most n_lanes entries
    std::future<ChunkIn> next_read = std::async(std::launch::async, read_chunk, std::cref(paths), std::cref(widths), std::cref(heights),
                                                (size_t)0, std::min(step, n));
    std::future<ChunkText> pending_art;
    std::shared_ptr<Stage> art_stage;                  // keeps the chunk alive while its artefacts are being written
    auto retire_oldest = [&]() {                       // device work of the oldest chunk is over: hand it to the artefact stage
        InFlight f = std::move(dev_q.front());
        dev_q.erase(dev_q.begin());
        f.done.get();
        std::shared_ptr<Stage> st = f.st;
        if (!st->dev_err.empty()) {
            // this chunk's images fail (message as process_single_image's); chunks already done keep their successes and
            // the chunks behind it still run
            const std::string msg = "Processing error: " + st->dev_err + " (files " + std::to_string(st->in.first) + ".." +
                                    std::to_string(st->in.first + st->in.count - 1) + " of the batch)";
            report(log_file, msg);
            return;
        }
        if (pending_art.valid()) emit(art_stage->in, art_stage->out, pending_art.get());
        art_stage = st;
        pending_art = std::async(std::launch::async, [st, &paths, &widths, &heights, &output_dir] {
            return artefact_chunk(st->in, st->out, paths, widths, heights, output_dir);
        });
    };
    size_t k = 0;
    for (size_t first = 0; first < n; first += step, ++k) {
        auto st = std::make_shared<Stage>();
        st->in = next_read.get();
        if (first + step < n)
            next_read = std::async(std::launch::async, read_chunk, std::cref(paths), std::cref(widths), std::cref(heights),
                                   first + step, std::min(step, n - first - step));
        for (size_t q = 0; q < st->in.count; ++q)
            if (!st->in.read_err[q].empty()) report(log_file, st->in.read_err[q]);
        if ((int)dev_q.size() == n_lanes) retire_oldest();          // frees the lane this chunk will use (FIFO: chunk k - n_lanes)
        mi_unet_group_t *lane = lanes[k % n_lanes];
        dev_q.push_back({ st, std::async(std::launch::async, [st, lane, &paths, &widths, &heights, &output_dir] {
            try {
                st->out = device_chunk(st->in, paths, widths, heights, output_dir, lane);
            } catch (const std::exception &e) {
                st->dev_err = e.what();
            }
            for (auto &r : st->in.raws) { g_pinned.release(r); r = PinnedPool::Buf{}; }     // the RAW images are on the device's side now
        }) });
    }
    while (!dev_q.empty()) retire_oldest();
    if (pending_art.valid()) emit(art_stage->in, art_stage->out, pending_art.get());
    return ok;
}

// ---- set_volume: the images of a batch as the slices of one volume.  process_images_targets fills the stack as its images finish;
// label_volume runs once, behind the last device call of the batch.
struct VolumeStack {
    // channel >= 0 (set_volume_measure): the stack also keeps that channel of every slice's normalised tile; texture_channel >= 0
    // (set_volume_texture) likewise, in a stack of its own only when the two channels differ
    VolumeStack(size_t slices, size_t targets, size_t hw, int channel = -1, int texture_channel = -1)
        : planes(targets * slices * hw, 0), intensity(channel >= 0 ? slices * hw : 0, 0),
          texture_own(texture_channel >= 0 && texture_channel != channel ? slices * hw : 0, 0), bases(slices), names(slices), D(slices), hw(hw),
          channel(channel), texture_channel(texture_channel)
    {
    }
    // image i of the batch is complete: plane t of its K final 0 / 255 pictures becomes slice i of target t; `tile` is its normalised
    // tile, [H][W][C]
    void add(size_t i, const std::string &base, const uint8_t *pictures, size_t K, const uint8_t *tile, size_t C)
    {
        for (size_t t = 0; t < K; ++t) std::copy(pictures + t * hw, pictures + (t + 1) * hw, planes.begin() + (t * D + i) * hw);
        if (channel >= 0 && (size_t)channel < C)
            for (size_t p = 0; p < hw; ++p) intensity[i * hw + p] = tile[p * C + (size_t)channel];
        if (!texture_own.empty() && (size_t)texture_channel < C)
            for (size_t p = 0; p < hw; ++p) texture_own[i * hw + p] = tile[p * C + (size_t)texture_channel];
        bases[i] = base;
    }
    const uint16_t *texture_intensity() const { return texture_own.empty() ? intensity.data() : texture_own.data(); }
    std::vector<uint8_t> planes;                       // [K][D][H][W]; a slice that failed stays all-zero
    std::vector<uint16_t> intensity;                   // [D][H][W] or empty: the measured channel of the normalised tiles, widened
    std::vector<uint16_t> texture_own;                 // [D][H][W] or empty: the texture's channel where it is not the measured one
    std::vector<std::string> bases, names;             // per slice: the base name once it is complete (else empty); the name it is reported by
    size_t D, hw;
    int channel, texture_channel;
};

// set_volume_clean: every target's plane of the stack through one mi_unet_volume_clean call with values = { 255 } on `h`
// (mi_unet_volume_clean_host under MEDSEG_HOST_POSTPROCESS=1), in place, before label_volume.  The integer units come from
// mi_unet_score_volume_units on the volume setting's spacing; a radius is llround(mm / unit_mm).  `json` receives the "clean" object of
// volume_report.json.  A failure is reported, leaves the stack as it was and returns false: the batch's volume stage ends there.
bool clean_volume(VolumeStack &st, const std::vector<mi_unet_target> &targets, const Volume &v, const VolumeClean &c, mi_unet_t *h,
                  std::ostream &lg, std::string &json)
{
    try {
        const size_t K = targets.size(), D = st.D, hw = st.hw;
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        int units[3] = { 0, 0, 0 };
        double unit_mm = 0.0;
        if (mi_unet_score_volume_units(spacing, (int)D, g_cfg.height, g_cfg.width, units, &unit_mm) != MI_UNET_OK)
            throw std::runtime_error(mi_unet_last_error());
        auto radius = [&](double mm, const char *which) {
            const double q = mm / unit_mm;
            if (!(q < 2147483647.0)) throw std::runtime_error(std::string(which) + " radius is out of range");     // (llround of it must fit an int)
            return (int)std::llround(q);
        };
        const mi_unet_volume_clean_opts opts{ c.fill ? 1 : 0, radius(c.close_mm, "close"), radius(c.open_mm, "open") };
        const int value = 255;
        const bool device = h && device_postprocess_requested();
        std::vector<uint8_t> cleaned(K * D * hw);
        std::vector<mi_unet_volume_clean_stat> stats(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const in = st.planes.data() + t * D * hw;
            uint8_t *const o = cleaned.data() + t * D * hw;
            const int rc = device ? mi_unet_volume_clean(h, in, (int)D, g_cfg.height, g_cfg.width, &value, 1, units, &opts, o, &stats[t])
                                  : mi_unet_volume_clean_host(in, (int)D, g_cfg.height, g_cfg.width, &value, 1, units, &opts, o, &stats[t]);
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
        }
        lg << "Volume clean: " << D << " slices, " << K << " targets, fill " << (c.fill ? "on" : "off") << ", close " << opts.close_r << ", open "
           << opts.open_r << " (unit " << unit_mm << " mm), " << ms_since(t0) << " ms" << std::endl;
        std::ostringstream js;
        js << "  \"clean\": {\"fill\": " << (c.fill ? "true" : "false") << ", \"close_mm\": " << json_number(c.close_mm) << ", \"open_mm\": "
           << json_number(c.open_mm) << ", \"unit_mm\": " << json_number(unit_mm) << ", \"close_r\": " << opts.close_r << ", \"open_r\": "
           << opts.open_r << ", \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            const mi_unet_volume_clean_stat &s = stats[t];
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"in_voxels\": " << s.in_voxels << ", \"filled\": " << s.filled
               << ", \"closed\": " << s.closed << ", \"opened\": " << s.opened << ", \"out_voxels\": " << s.out_voxels << "}";
        }
        js << "\n  ]},\n";
        json = js.str();
        st.planes.swap(cleaned);
        return true;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume clean error: ") + e.what());
        return false;
    }
}

// set_volume_mesh: every target's plane of `planes` ([K][D][H][W], the stack label_volume labelled) through mi_unet_volume_mesh with
// values = { 255 } on `h` (mi_unet_volume_mesh_host under MEDSEG_HOST_POSTPROCESS=1) -- a counting call, then one sized by its counts --
// then the positions and metrics under the volume setting's spacing and the STL file of every target that has quads.  Returns the
// "mesh" member of volume_report.json, from its leading comma on.  A failure is reported and returns an empty text: only this step ends.
std::string mesh_volume(const uint8_t *planes, size_t D, size_t hw, const std::vector<mi_unet_target> &targets, const Volume &v, const VolumeMesh &mesh,
                        mi_unet_t *h, const std::string &output_dir, std::ostream &lg)
{
    try {
        const size_t K = targets.size();
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        const int value = 255;
        const bool device = h && device_postprocess_requested();
        const char *const placement = mesh.placement == MI_UNET_MESH_NETS ? "nets" : "faces";
        std::ostringstream js;
        js << ",\n  \"mesh\": {\"placement\": \"" << placement << "\", \"targets\": [";
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const in = planes + t * D * hw;
            auto call = [&](mi_unet_mesh_vertex *verts, int cap_verts, int32_t *quads, int cap_quads, mi_unet_mesh_stat *st) {
                const int rc = device ? mi_unet_volume_mesh(h, in, (int)D, g_cfg.height, g_cfg.width, &value, 1, mesh.placement, verts, cap_verts, quads,
                                                            cap_quads, st)
                                      : mi_unet_volume_mesh_host(in, (int)D, g_cfg.height, g_cfg.width, &value, 1, mesh.placement, verts, cap_verts,
                                                                 quads, cap_quads, st);
                if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            };
            mi_unet_mesh_stat st{};
            call(nullptr, 0, nullptr, 0, &st);
            std::vector<mi_unet_mesh_vertex> verts((size_t)st.verts);
            std::vector<int32_t> quads((size_t)st.quads * 4);
            if (st.quads > 0) call(verts.data(), (int)st.verts, quads.data(), (int)st.quads, &st);
            mi_unet_mesh_metrics m{};
            if (mi_unet_volume_mesh_derive(verts.data(), (int)verts.size(), quads.data(), (int)st.quads, spacing, &m) != MI_UNET_OK)
                throw std::runtime_error(mi_unet_last_error());
            std::string file;
            if (st.quads > 0) {
                std::vector<float> xyz(verts.size() * 3);
                if (mi_unet_volume_mesh_positions(verts.data(), (int)verts.size(), spacing, xyz.data()) != MI_UNET_OK)
                    throw std::runtime_error(mi_unet_last_error());
                file = is_default(targets) ? "volume_mesh.stl" : "volume_mesh_class" + std::to_string(targets[t].cls) + ".stl";
                VolumeMeshArtefact a;
                a.output_dir = output_dir; a.file = file; a.xyz = xyz.data(); a.quads = quads.data(); a.nv = verts.size(); a.nq = (size_t)st.quads;
                write_volume_mesh(a);
            }
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"quads\": " << st.quads << ", \"verts\": " << st.verts
               << ", \"area_mm2\": " << json_number(m.area_mm2) << ", \"volume_mm3\": " << json_number(m.volume_mm3) << ", \"file\": "
               << (file.empty() ? std::string("null") : "\"" + file + "\"") << "}";
        }
        js << "\n  ]}";
        lg << "Volume mesh: " << D << " slices, " << K << " targets, " << placement << ", " << ms_since(t0) << " ms" << std::endl;
        return js.str();
    } catch (const std::exception &e) {
        report(lg, std::string("Volume mesh error: ") + e.what());
        return std::string();
    }
}

// set_volume_measure: per target one mi_unet_volume_measure call on `h` (mi_unet_volume_measure_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's intensity, with m = min(found, cap) and the integer units of
// mi_unet_score_volume_units for the volume setting's spacing.  Returns, per target and table row, the "measure" member of the row's
// component object in volume_report.json, from its leading comma on.  A failure is reported and returns nothing: only this step ends.
std::vector<std::vector<std::string>> measure_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found,
                                                     size_t cap, const std::vector<mi_unet_target> &targets, const Volume &v,
                                                     const VolumeMeasure &measure, mi_unet_t *h, std::ostream &lg)
{
    try {
        const size_t K = targets.size(), D = st.D, hw = st.hw;
        const int W = g_cfg.width;
        if (measure.channel >= g_cfg.in_ch)
            throw std::runtime_error("channel " + std::to_string(measure.channel) + " of " + std::to_string(g_cfg.in_ch));
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        int units[3] = { 0, 0, 0 };
        double unit_mm = 0.0;
        if (mi_unet_score_volume_units(spacing, (int)D, g_cfg.height, g_cfg.width, units, &unit_mm) != MI_UNET_OK)
            throw std::runtime_error(mi_unet_last_error());
        const mi_unet_vmeasure_opts opts{ measure.max_ends };
        const bool device = h && device_postprocess_requested();
        std::vector<std::vector<std::string>> members(K);
        auto point = [&](int32_t idx) {
            const size_t p = (size_t)idx % hw;
            return "[" + std::to_string(p % (size_t)W) + ", " + std::to_string(p / (size_t)W) + ", " + std::to_string((size_t)idx / hw) + "]";
        };
        auto ends = [&](int32_t p, int32_t q) { return "[" + point(p) + ", " + point(q) + "]"; };
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const int m = (int)std::min<size_t>((size_t)found[t], cap);
            if (m < 1) continue;
            std::vector<mi_unet_vmeasure> table((size_t)m);
            const int32_t *const in = ids.data() + t * D * hw;
            const int rc = device ? mi_unet_volume_measure(h, in, st.intensity.data(), (int)D, g_cfg.height, g_cfg.width, m, units, &opts, table.data())
                                  : mi_unet_volume_measure_host(in, st.intensity.data(), (int)D, g_cfg.height, g_cfg.width, m, units, &opts, table.data());
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            for (const mi_unet_vmeasure &c : table) {
                if (c.voxels < 1) {                             // dropped by the volume filter: its voxels carry no id
                    members[t].push_back(", \"measure\": null");
                    continue;
                }
                mi_unet_vmeasure_shape s{};
                if (mi_unet_volume_measure_derive(&c, units, unit_mm, &s) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
                const bool searched = c.d2 >= 0;
                std::ostringstream js;
                js << ", \"measure\": {\"diameter_mm\": " << (searched ? json_number(s.diameter_mm) : "null") << ", \"diameter_ends\": "
                   << (searched ? ends(c.dp, c.dq) : "null") << ", \"axial_diameter_mm\": " << (searched ? json_number(s.axial_diameter_mm) : "null")
                   << ", \"axial_slice\": " << (searched ? "\"" + medseg::json_escape(st.names[(size_t)c.a_p / hw]) + "\"" : std::string("null"))
                   << ", \"axial_ends\": " << (searched ? ends(c.a_p, c.a_q) : "null") << ", \"axes_mm\": [" << json_number(s.axis_mm[0]) << ", "
                   << json_number(s.axis_mm[1]) << ", " << json_number(s.axis_mm[2]) << "], \"axes_dir\": [";
                for (int i = 0; i < 3; ++i)
                    js << (i ? ", " : "") << "[" << json_number(s.axis_dir[i][0]) << ", " << json_number(s.axis_dir[i][1]) << ", "
                       << json_number(s.axis_dir[i][2]) << "]";
                js << "], \"mean\": " << json_number(s.mean) << ", \"std\": " << json_number(s.std) << ", \"min\": " << c.imin << ", \"max\": "
                   << c.imax << ", \"ends\": " << c.ends << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume measure: " << D << " slices, " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume measure error: ") + e.what());
        return {};
    }
}

// set_volume_texture: per target one mi_unet_volume_texture call on `h` (mi_unet_volume_texture_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's texture channel, with m = min(found, cap, 2^22 / levels^2), then
// mi_unet_volume_texture_derive of every row and of both its tables.  Returns, per target and table row, the "texture" member of the row's
// component object in volume_report.json, from its leading comma on.  A failure is reported and returns nothing: only this step ends.
std::vector<std::vector<std::string>> texture_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found,
                                                     size_t cap, const std::vector<mi_unet_target> &targets, const VolumeTexture &texture,
                                                     mi_unet_t *h, std::ostream &lg)
{
    try {
        const size_t K = targets.size(), D = st.D, hw = st.hw, L = (size_t)texture.levels;
        if (texture.channel >= g_cfg.in_ch)
            throw std::runtime_error("channel " + std::to_string(texture.channel) + " of " + std::to_string(g_cfg.in_ch));
        const mi_unet_vtexture_opts opts{ texture.mode, texture.levels, texture.lo, texture.width };
        const bool device = h && device_postprocess_requested();
        const size_t most = (size_t)MI_UNET_VTEX_MAX_CELLS / (L * L);
        std::vector<std::vector<std::string>> members(K);
        size_t cut = 0;                                         // components beyond the measured count, over all targets
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const size_t rows = std::min<size_t>((size_t)found[t], cap);
            const int m = (int)std::min(rows, most);
            if (m < 1) continue;
            cut += rows - (size_t)m;
            std::vector<mi_unet_vtexture> table((size_t)m);
            std::vector<uint32_t> hist((size_t)m * L), glcm((size_t)m * L * L), axial((size_t)m * L * L);
            const int32_t *const in = ids.data() + t * D * hw;
            const int rc = device ? mi_unet_volume_texture(h, in, st.texture_intensity(), (int)D, g_cfg.height, g_cfg.width, m, &opts, table.data(),
                                                           hist.data(), glcm.data(), axial.data())
                                  : mi_unet_volume_texture_host(in, st.texture_intensity(), (int)D, g_cfg.height, g_cfg.width, m, &opts, table.data(),
                                                                hist.data(), glcm.data(), axial.data());
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            for (size_t r = 0; r < rows; ++r) {
                if (r >= (size_t)m || table[r].voxels < 1) {    // beyond the measured count, or dropped by the volume filter: no voxel carries its id
                    members[t].push_back(", \"texture\": null");
                    continue;
                }
                const mi_unet_vtexture &c = table[r];
                mi_unet_vtexture_features f{}, fa{};
                if (mi_unet_volume_texture_derive(&c, hist.data() + r * L, glcm.data() + r * L * L, (int)L, &f) != MI_UNET_OK ||
                    mi_unet_volume_texture_derive(&c, hist.data() + r * L, axial.data() + r * L * L, (int)L, &fa) != MI_UNET_OK)
                    throw std::runtime_error(mi_unet_last_error());
                std::ostringstream js;
                js << ", \"texture\": {\"levels\": " << L << ", \"mode\": \"" << (texture.mode == MI_UNET_VTEX_WIDTH ? "width" : "count")
                   << "\", \"range\": [" << c.imin << ", " << c.imax << "], \"levels_used\": " << c.levels_used << ", \"histogram\": {\"mean\": "
                   << json_number(f.mean) << ", \"variance\": " << json_number(f.variance) << ", \"skewness\": " << json_number(f.skewness) << ", \"kurtosis\": "
                   << json_number(f.kurtosis) << ", \"median\": " << f.median << ", \"p10\": " << f.p10 << ", \"p90\": " << f.p90 << ", \"mode\": "
                   << f.mode << ", \"entropy\": " << json_number(f.entropy) << ", \"uniformity\": " << json_number(f.uniformity) << ", \"counts\": [";
                for (size_t l = 0; l < L; ++l) js << (l ? ", " : "") << hist[r * L + l];
                js << "]}";
                auto joint = [&](const char *key, int64_t pairs, const mi_unet_vtexture_features &g) {
                    js << ", \"" << key << "\": {\"pairs\": " << pairs << ", \"joint_max\": " << json_number(g.joint_max) << ", \"joint_average\": "
                       << json_number(g.joint_average) << ", \"joint_variance\": " << json_number(g.joint_variance) << ", \"joint_entropy\": "
                       << json_number(g.joint_entropy) << ", \"contrast\": " << json_number(g.contrast) << ", \"dissimilarity\": " << json_number(g.dissimilarity)
                       << ", \"inverse_difference\": " << json_number(g.inverse_difference) << ", \"inverse_difference_moment\": "
                       << json_number(g.inverse_difference_moment) << ", \"angular_second_moment\": " << json_number(g.angular_second_moment)
                       << ", \"correlation\": " << json_number(g.correlation) << "}";
                };
                joint("glcm", c.pairs, f);
                joint("glcm_axial", c.pairs_axial, fa);
                js << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume texture: " << D << " slices, " << K << " targets, " << ms_since(t0) << " ms";
        if (cut) lg << " (the first " << most << " components of a target at " << L << " levels; " << cut << " not measured)";
        lg << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume texture error: ") + e.what());
        return {};
    }
}

// One mi_unet_volume_components call per target with values = { 255 } on `h` (mi_unet_volume_components_host under
// MEDSEG_HOST_POSTPROCESS=1), then volume_report.json and, under a filter, the <base>_volume_mask pictures.  A failure is reported and
// fails no image.  Under a filter `filtered` receives the filtered stack [K][D][H][W]; it stays empty without one, or after a failure.
// A stack that clean_volume cleaned comes with its "clean" object for the report and is written as pictures whether or not a filter
// is active (without one they are the cleaned stack itself).  With `mesh` on, the planes that were labelled -- `out` under a filter, else
// the stack -- are meshed (mesh_volume) and the report gains the "mesh" object behind "targets".  With `measure` on, the components
// stage also hands out its ids, they are measured (measure_volume) and every component object gains a last member "measure".  With
// `texture` on, the ids are handed out likewise and every component object gains a last member "texture" (texture_volume).  With
// `numbered` given (set_volume_match) the ids [K][D][H][W] and the counts per target are handed out too; it stays empty after a failure.
struct VolumeIds {
    std::vector<int32_t> ids, found;
};
void label_volume(const VolumeStack &st, const std::vector<mi_unet_target> &targets, const Volume &v, mi_unet_t *h, const std::string &output_dir,
                  std::ostream &lg, std::vector<uint8_t> &filtered, const std::string &clean_json = std::string(),
                  const VolumeMesh &mesh = VolumeMesh(), const VolumeMeasure &measure = VolumeMeasure(), VolumeIds *numbered = nullptr,
                  const VolumeTexture &texture = VolumeTexture())
{
    filtered.clear();
    try {
        const size_t K = targets.size(), D = st.D, hw = st.hw, cap = MI_UNET_VOLUME_MAX_TABLE;
        const bool filter = v.min_voxels > 0 || v.keep_largest > 0 || !clean_json.empty();
        std::vector<uint8_t> out(filter ? K * D * hw : 0);
        std::vector<mi_unet_vcomp> table(K * cap);
        std::vector<int32_t> found(K), kept(K), ids(measure.on || texture.on || numbered ? K * D * hw : 0);
        const mi_unet_volume_opts opts{ v.connectivity, v.min_voxels, v.keep_largest };
        const int value = 255;
        const bool device = h && device_postprocess_requested();
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const in = st.planes.data() + t * D * hw;
            uint8_t *const o = filter ? out.data() + t * D * hw : nullptr;
            int32_t *const id = ids.empty() ? nullptr : ids.data() + t * D * hw;
            const int rc = device ? mi_unet_volume_components(h, in, (int)D, g_cfg.height, g_cfg.width, &value, 1, &opts, o, id,
                                                              table.data() + t * cap, (int)cap, &found[t], &kept[t])
                                  : mi_unet_volume_components_host(in, (int)D, g_cfg.height, g_cfg.width, &value, 1, &opts, o, id,
                                                                   table.data() + t * cap, (int)cap, &found[t], &kept[t]);
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
        }
        lg << "Volume: " << D << " slices, " << K << " targets, connectivity " << v.connectivity << ", " << ms_since(t0) << " ms" << std::endl;
        const std::string mesh_json = mesh.on ? mesh_volume(filter ? out.data() : st.planes.data(), D, hw, targets, v, mesh, h, output_dir, lg) : std::string();
        const std::vector<std::vector<std::string>> measured =
            measure.on ? measure_volume(st, ids, found, cap, targets, v, measure, h, lg) : std::vector<std::vector<std::string>>();
        const std::vector<std::vector<std::string>> textured =
            texture.on ? texture_volume(st, ids, found, cap, targets, texture, h, lg) : std::vector<std::vector<std::string>>();
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        std::ostringstream js;
        auto names = [&](const char *key, bool missing) {
            js << "  \"" << key << "\": [";
            bool first = true;
            for (size_t z = 0; z < D; ++z) {
                if (missing && !st.bases[z].empty()) continue;
                js << (first ? "" : ", ") << "\"" << medseg::json_escape(st.names[z]) << "\"";
                first = false;
            }
            js << "],\n";
        };
        js << "{\n";
        names("slices", false);
        names("missing", true);
        js << "  \"connectivity\": " << v.connectivity << ",\n  \"min_voxels\": " << v.min_voxels << ",\n  \"keep_largest\": " << v.keep_largest
           << ",\n  \"spacing\": [" << json_number(spacing[0]) << ", " << json_number(spacing[1]) << ", " << json_number(spacing[2])
           << "],\n" << clean_json << "  \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"found\": " << found[t] << ", \"kept\": " << kept[t]
               << ", \"components\": [";
            const size_t rows = std::min<size_t>((size_t)found[t], cap);
            for (size_t r = 0; r < rows; ++r) {
                const mi_unet_vcomp &c = table[t * cap + r];
                mi_unet_vcomp_metrics m{};
                if (mi_unet_volume_derive(&c, spacing, &m) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
                js << (r ? "," : "") << "\n      {\"voxels\": " << c.voxels << ", \"kept\": " << c.kept << ", \"bbox\": [" << c.x0 << ", " << c.y0 << ", "
                   << c.z0 << ", " << c.x1 << ", " << c.y1 << ", " << c.z1 << "], \"centroid_mm\": [" << json_number(m.cx_mm) << ", "
                   << json_number(m.cy_mm) << ", " << json_number(m.cz_mm) << "], \"volume_mm3\": " << json_number(m.volume_mm3)
                   << ", \"surface_mm2\": " << json_number(m.surface_mm2) << ", \"extent_mm\": [" << json_number(m.extent_x_mm) << ", "
                   << json_number(m.extent_y_mm) << ", " << json_number(m.extent_z_mm) << "]" << (measured.empty() ? std::string() : measured[t][r])
                   << (textured.empty() ? std::string() : textured[t][r]) << "}";
            }
            js << (rows ? "\n    " : "") << "]}";
        }
        js << "\n  ]" << mesh_json << "\n}\n";
        VolumeArtefacts a;
        a.output_dir = output_dir; a.report = js.str(); a.targets = &targets; a.bases = &st.bases; a.out = filter ? out.data() : nullptr;
        a.height = g_cfg.height; a.width = g_cfg.width;
        write_volume_artefacts(a);
        filtered.swap(out);
        if (numbered) {
            numbered->ids.swap(ids);
            numbered->found.swap(found);
        }
    } catch (const std::exception &e) {
        report(lg, std::string("Volume error: ") + e.what());
    }
}

// set_volume_match: per target the truth stack (0 / 255, [D][H][W] at truth_planes + t * D * hw) labelled by mi_unet_volume_components
// under the setting's connectivity, no filter and a table of MI_UNET_VOLUME_MAX_TABLE, then one mi_unet_volume_match call on `h`
// (the host forms under MEDSEG_HOST_POSTPROCESS=1) against the ids label_volume numbered, mi_unet_volume_match_assign at the setting's
// threshold and mi_unet_volume_match_derive.  Returns per target the "lesions" member of its object in volume_score.json, from its
// leading comma on.  A failure is reported and returns nothing: only this step ends.
std::vector<std::string> match_volume(const VolumeIds &numbered, const std::vector<uint8_t> &truth_planes, size_t D, size_t hw,
                                      const std::vector<mi_unet_target> &targets, const Volume &v, const VolumeMatch &match, mi_unet_t *h,
                                      std::ostream &lg)
{
    try {
        const size_t K = targets.size(), table_cap = MI_UNET_VOLUME_MAX_TABLE;
        if (numbered.ids.size() != K * D * hw || numbered.found.size() != K) throw std::runtime_error("the labelled stack is missing");
        const bool device = h && device_postprocess_requested();
        const mi_unet_volume_opts opts{ v.connectivity, 0, 0 };
        const int value = 255;
        std::vector<std::string> members(K);
        std::vector<int32_t> truth_ids(D * hw);
        std::vector<mi_unet_vcomp> truth_table(table_cap);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const truth = truth_planes.data() + t * D * hw;
            int32_t truth_found = 0, truth_kept = 0;
            int rc = device ? mi_unet_volume_components(h, truth, (int)D, g_cfg.height, g_cfg.width, &value, 1, &opts, nullptr, truth_ids.data(),
                                                        truth_table.data(), (int)table_cap, &truth_found, &truth_kept)
                            : mi_unet_volume_components_host(truth, (int)D, g_cfg.height, g_cfg.width, &value, 1, &opts, nullptr, truth_ids.data(),
                                                             truth_table.data(), (int)table_cap, &truth_found, &truth_kept);
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            const size_t mp = std::min<size_t>((size_t)numbered.found[t], table_cap), mt = std::min<size_t>((size_t)truth_found, table_cap);
            const bool truncated = (size_t)numbered.found[t] > table_cap || (size_t)truth_found > table_cap;
            // a side without components is matched as one id that no voxel carries: an all-zero entry, which is not present
            const size_t np = std::max<size_t>(mp, 1), nt = std::max<size_t>(mt, 1);
            const size_t cap = std::min(np * nt, D * hw);       // a pair holds a cell and a voxel of its own: the list is never truncated
            std::vector<mi_unet_vmatch_side> ps(np), ts(nt);
            std::vector<mi_unet_vmatch_pair> pairs(cap);
            int found = 0;
            const int32_t *const pred_ids = numbered.ids.data() + t * D * hw;
            rc = device ? mi_unet_volume_match(h, pred_ids, truth_ids.data(), (int)D, g_cfg.height, g_cfg.width, (int)np, (int)nt, (int)cap, ps.data(),
                                               ts.data(), pairs.data(), &found)
                        : mi_unet_volume_match_host(pred_ids, truth_ids.data(), (int)D, g_cfg.height, g_cfg.width, (int)np, (int)nt, (int)cap, ps.data(),
                                                    ts.data(), pairs.data(), &found);
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            std::vector<int32_t> of_p(np), of_t(nt);
            mi_unet_vmatch_counts c{};
            mi_unet_vmatch_scores sc{};
            if (mi_unet_volume_match_assign(ps.data(), (int)np, ts.data(), (int)nt, pairs.data(), found, (int)cap, match.iou_num, match.iou_den,
                                            of_p.data(), of_t.data(), &c) != MI_UNET_OK ||
                mi_unet_volume_match_derive(ps.data(), (int)np, ts.data(), (int)nt, pairs.data(), found, (int)cap, of_p.data(), &sc) != MI_UNET_OK)
                throw std::runtime_error(mi_unet_last_error());
            std::ostringstream js;
            js << ", \"lesions\": {\"pred\": " << mp << ", \"truth\": " << mt << ", \"iou_threshold\": [" << match.iou_num << ", " << match.iou_den
               << "], \"tp\": " << c.tp << ", \"fp\": " << c.fp << ", \"fn\": " << c.fn << ", \"precision\": " << json_number(sc.precision)
               << ", \"recall\": " << json_number(sc.recall) << ", \"f1\": " << json_number(sc.f1) << ", \"pq\": " << json_number(sc.pq)
               << ", \"sq\": " << json_number(sc.sq) << ", \"rq\": " << json_number(sc.rq) << ", \"mean_dice\": " << json_number(sc.mean_dice)
               << ", \"matches\": [";
            bool first = true;
            for (size_t r = 0; r < mp; ++r) {
                if (!of_p[r]) continue;
                const int32_t tc = of_p[r] - 1;
                const mi_unet_vmatch_pair *q = pairs.data();
                while (q->p != (int32_t)r || q->t != tc) ++q;   // (derive has found it: the match is in the list)
                const double i = q->voxels, vp = ps[r].voxels, vt = ts[tc].voxels;
                js << (first ? "" : ", ") << "{\"pred\": " << r << ", \"truth\": " << tc << ", \"voxels\": " << q->voxels << ", \"iou\": "
                   << json_number(i / (vp + vt - i)) << ", \"dice\": " << json_number(2.0 * i / (vp + vt)) << ", \"pred_voxels\": " << ps[r].voxels
                   << ", \"truth_voxels\": " << ts[tc].voxels << "}";
                first = false;
            }
            js << "], \"missed\": [";
            first = true;
            for (size_t k = 0; k < mt; ++k) {
                if (of_t[k] || ts[k].voxels < 1) continue;
                js << (first ? "" : ", ") << "{\"truth\": " << k << ", \"voxels\": " << ts[k].voxels << "}";
                first = false;
            }
            js << "], \"spurious\": [";
            first = true;
            for (size_t r = 0; r < mp; ++r) {
                if (of_p[r] || ps[r].voxels < 1) continue;
                js << (first ? "" : ", ") << r;
                first = false;
            }
            js << "]" << (truncated ? ", \"truncated\": true" : "") << "}";
            members[t] = js.str();
        }
        lg << "Volume match: " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume match error: ") + e.what());
        return {};
    }
}

// set_volume with set_truth_dir: the stack against <dir>/<base>_labels.raw of every slice as ONE volume (mi_unet_score_volume in
// include/mi_unet.h).  One call per target with values = { 255 } on `h` (mi_unet_score_volume_host under
// MEDSEG_HOST_POSTPROCESS=1): pred is the target's plane of `filtered` when the volume filter is active, else of the stack; truth is
// recoded to 0 / 255 by truth == cls.  The integer units come from mi_unet_score_volume_units on the setting's spacing.  Writes
// <output_dir>/volume_score.json.  Only a stack whose every slice completed and has a truth file of the tile's size is scored; a
// failure is reported and fails no image.  With `match` on, every target object gains a last member "lesions" (match_volume) from the
// ids label_volume numbered.
void score_volume_stack(const VolumeStack &st, const std::vector<uint8_t> &filtered, const std::vector<mi_unet_target> &targets, const Volume &v,
                        const std::string &truth_dir, mi_unet_t *h, const std::string &output_dir, std::ostream &lg,
                        const VolumeMatch &match = VolumeMatch(), const VolumeIds &numbered = VolumeIds())
{
    try {
        const size_t K = targets.size(), D = st.D, hw = st.hw;
        const bool filter = !filtered.empty() || v.min_voxels > 0 || v.keep_largest > 0;       // (a cleaned stack comes filtered too)
        if (filter && filtered.size() != K * D * hw) throw std::runtime_error("the filtered stack is missing");
        std::vector<uint8_t> labels(D * hw), truth(D * hw), truth_planes(match.on ? K * D * hw : 0);
        size_t without = 0;
        for (size_t z = 0; z < D; ++z) {
            bool good = !st.bases[z].empty();
            if (good) {
                const std::string path = truth_dir + "/" + st.bases[z] + "_labels.raw";
                std::error_code ec;
                const auto size = fs::file_size(path, ec);
                std::ifstream f(path, std::ios::binary);
                good = !ec && size == hw && f.read(reinterpret_cast<char *>(labels.data() + z * hw), (std::streamsize)hw);
            }
            without += !good;
        }
        if (without) {
            lg << "Volume score skipped: " << without << " of " << D << " slices without mask or truth" << std::endl;
            return;
        }
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        int units[3] = { 0, 0, 0 };
        double unit_mm = 0.0;
        if (mi_unet_score_volume_units(spacing, (int)D, g_cfg.height, g_cfg.width, units, &unit_mm) != MI_UNET_OK)
            throw std::runtime_error(mi_unet_last_error());
        const mi_unet_score_opts opts{ 50000, 0 };
        const int value = 255;
        const bool device = h && device_postprocess_requested();
        std::vector<mi_unet_score> scores(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const pred = (filter ? filtered.data() : st.planes.data()) + t * D * hw;
            for (size_t i = 0; i < D * hw; ++i) truth[i] = labels[i] == targets[t].cls ? 255 : 0;
            const int rc = device ? mi_unet_score_volume(h, pred, truth.data(), (int)D, g_cfg.height, g_cfg.width, &value, 1, units, &opts, &scores[t],
                                                         nullptr, nullptr)
                                  : mi_unet_score_volume_host(pred, truth.data(), (int)D, g_cfg.height, g_cfg.width, &value, 1, units, &opts,
                                                              &scores[t], nullptr, nullptr);
            if (rc != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            if (match.on) std::copy(truth.begin(), truth.end(), truth_planes.begin() + t * D * hw);
        }
        lg << "Volume score: " << D << " slices, " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        const std::vector<std::string> lesions = match.on ? match_volume(numbered, truth_planes, D, hw, targets, v, match, h, lg) : std::vector<std::string>();
        std::ostringstream js;
        js << "{\n  \"slices\": [";
        for (size_t z = 0; z < D; ++z) js << (z ? ", " : "") << "\"" << medseg::json_escape(st.names[z]) << "\"";
        js << "],\n  \"unit_mm\": " << json_number(unit_mm) << ",\n  \"spacing_units\": [" << units[0] << ", " << units[1] << ", " << units[2]
           << "],\n  \"quantile_ppm\": " << opts.quantile_ppm << ",\n  \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            const mi_unet_score &sc = scores[t];
            mi_unet_score_metrics m{};
            if (mi_unet_score_volume_derive(&sc, unit_mm, &m) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"tp\": " << sc.tp << ", \"fp\": " << sc.fp << ", \"fn\": " << sc.fn
               << ", \"dice\": " << json_number(m.dice) << ", \"iou\": " << json_number(m.iou) << ", \"hd_mm\": " << json_number(m.hd)
               << ", \"hd_q_mm\": " << json_number(m.hd_q) << ", \"assd_mm\": " << json_number(m.assd) << ", \"rmsd_mm\": " << json_number(m.rmsd)
               << (lesions.empty() ? std::string() : lesions[t]) << "}";
        }
        js << "\n  ]\n}\n";
        write_volume_score(output_dir, js.str());
    } catch (const std::exception &e) {
        report(lg, std::string("Volume score error: ") + e.what());
    }
}

// ---- a non-default target list (set_targets) or morphology (set_morphology): K masks per image, named <base>_mask_class<cls>.png, or
// under the default target list the one <base>_mask.png.  One plain route for both entry points: read the files of a chunk,
// one device call for the chunk (mi_unet_segment_raw16_multi on `ctx`, or its group form when ctx is null), then the artefacts image
// by image.  With MEDSEG_HOST_POSTPROCESS / _CONTOURS = 1 the device call ends at the label maps and the CPU chain (postprocess_mask
// per target, mask picture, extract_contours) takes over; MEDSEG_HOST_PREPROCESS has no effect here (the device's tile is the CPU's
// bit for bit).  Returns the number of images that succeeded.
int process_images_targets(const std::vector<std::string> &paths, const std::vector<int> &widths, const std::vector<int> &heights,
                           const std::string &output_dir, mi_unet_t *ctx, const std::vector<mi_unet_target> &targets,
                           const std::vector<mi_unet_morph> &morph, std::ostream &lg, VolumeStack *volume = nullptr)
{
    const size_t n = paths.size(), hw = (size_t)g_cfg.height * g_cfg.width, K = targets.size();
    if (morph.size() != 1 && morph.size() != K)
        throw std::runtime_error("the morphology list has " + std::to_string(morph.size()) + " entries, the target list " + std::to_string(K));
    const int C = g_cfg.in_ch;
    const Device dev{ ctx, ctx ? nullptr : get_engine_group() };
    if (!ctx && !dev.group) throw std::runtime_error("Engine not initialized");
    const bool device_tail = device_postprocess_requested() && device_contours_requested();
    const size_t step = ctx ? 1 : (size_t)std::max(1, g_cfg.max_batch) * (size_t)std::max(1, mi_unet_group_size(dev.group));
    int ok = 0;
    for (size_t first = 0; first < n; first += step) {
        const size_t count = std::min(step, n - first);
        std::vector<std::vector<uint16_t>> raws(count);
        RawArgs args;
        std::vector<size_t> idx;
        for (size_t k = 0; k < count; ++k) {
            const size_t i = first + k;
            auto read = [&] { return Preprocess::read_raw16(paths[i], widths[i], heights[i]); };
            try {
                raws[k] = ctx ? read_or_fail(read) : read();
            } catch (const std::exception &e) {
                if (ctx) throw;
                report(lg, std::string("Processing error: ") + e.what() + " (" + paths[i] + ")");
                continue;
            }
            args.add(raws[k].data(), widths[i], heights[i]);
            idx.push_back(i);
        }
        const size_t m = idx.size();
        if (m == 0) continue;
        std::vector<uint8_t> tiles(hw * m * C), masks(hw * m * K), labels(device_tail ? 0 : hw * m);
        std::vector<int32_t> xy(device_tail ? m * K * (size_t)kCapPoints * 2 : 0), start(m * K * (kCapContours + 1)), cnt(m * K, -1);
        const auto t0 = hr_clock::now();
        const int rc = device_tail ? dev.segment_raw16_multi(args, tiles.data(), masks.data(), xy.data(), start.data(), cnt.data())
                                   : dev.infer_raw16(args, tiles.data(), labels.data());
        if (rc != MI_UNET_OK) throw std::runtime_error(std::string("Inference failed: ") + mi_unet_last_error());
        const RegionReport regions = device_tail ? RegionReport(dev, m * K) : RegionReport();
        lg << "Inference time: " << ms_since(t0) << " ms" << (m > 1 ? " for " + std::to_string(m) + " images" : std::string()) << std::endl;
        std::vector<std::string> scored(m);            // set_truth_dir: the images whose masks are complete
        for (size_t k = 0; k < m; ++k) {
            const size_t i = idx[k];
            const std::string base_name = fs::path(paths[i]).stem().string();
            try {
                if (!ctx) lg << "\n=== Processing Image: " << fs::path(paths[i]).filename().string() << " ===" << std::endl;
                Image8 tile(g_cfg.height, g_cfg.width, 1);
                keep_channel0(&tiles[k * hw * C], hw, C, tile.data.data());
                std::vector<Image8> vis(K);
                std::vector<PlaneShapes> shapes(K);    // (the host chain leaves cnt at -1 and xy empty: the host tracer)
                for (size_t t = 0; t < K; ++t) {
                    const size_t plane = k * K + t;
                    if (device_tail) {
                        vis[t] = tile_image(masks, plane);
                    } else {
                        vis[t] = Image8(g_cfg.height, g_cfg.width, 1);
                        const Image8 pm = postprocess_mask(tile_image(labels, k), targets[t].cls, targets[t].min_area_frac,
                                                           morph[morph.size() == 1 ? 0 : t]);
                        for (size_t p = 0; p < hw; ++p) vis[t].data[p] = pm.data[p] ? 255 : 0;
                        std::copy(vis[t].data.begin(), vis[t].data.end(), masks.begin() + plane * hw);
                    }
                    shapes[t] = { xy.data() + (device_tail ? plane * (size_t)kCapPoints * 2 : 0), &start[plane * (kCapContours + 1)], cnt[plane],
                                  regions.of(plane, cnt[plane]) };
                }
                ImageArtefacts a;
                a.tile = &tile; a.targets = &targets; a.masks = vis.data(); a.planes = shapes.data(); a.width = widths[i]; a.height = heights[i];
                a.raw_path = paths[i]; a.output_dir = output_dir; a.base_name = base_name; a.console = &std::cout; a.class_lines = true;
                write_image_artefacts(a);
                if (!ctx) lg << "Processing completed for: " << base_name << std::endl;
                scored[k] = base_name;
                if (volume) volume->add(i, base_name, &masks[k * K * hw], K, &tiles[k * hw * C], (size_t)C);
                ++ok;
            } catch (const std::exception &e) {
                if (ctx) throw;
                report(lg, std::string("Processing error: ") + e.what());
            }
        }
        // one scoring call for the images of this device call (the group's first engine: the caller holds the batch lock)
        score_and_note(ctx ? ctx : mi_unet_group_handle(dev.group, 0), scored, masks.data(), targets, output_dir, lg);
    }
    return ok;
}

}  // namespace

void release_pinned_buffers() { g_pinned.clear(); }

// Device-first form of the pipeline for N images at once (the reference loops files one by one, src/main.cpp:148-164).
// All-device route (default): the chunked three-stage pipeline above.  With MEDSEG_HOST_POSTPROCESS / _CONTOURS = 1:
// RAW16 -> [device: min/max, bilinear resample, quantise, UNet, argmax] -> per image on the host: PNG/JSON artefacts,
// postprocess_mask, contours.  Returns the number of images that succeeded.
int process_image_batch(const std::vector<std::string> &raw_paths, const std::vector<int> &widths,
                        const std::vector<int> &heights, const std::string &output_dir)
{
    std::ostream &log_file = log_or_nothing();
    int ok = 0;
    try {
        mi_unet_group_t *group = get_engine_group();
        if (!group) throw std::runtime_error("Engine not initialized");
        const size_t n = raw_paths.size();
        if (widths.size() != n || heights.size() != n) throw std::runtime_error("widths/heights do not match raw_paths");
        const Settings settings = current_settings();
        if (settings.volume.on && n > 0) {                     // the paths are the slices of one volume, whatever the target list is
            std::lock_guard<std::mutex> lk(g_batch_mutex);
            Collected lg{ log_file, {} };
            VolumeStack stack(n, settings.targets.size(), (size_t)g_cfg.height * g_cfg.width, settings.volume_measure.on ? settings.volume_measure.channel : -1,
                              settings.volume_texture.on ? settings.volume_texture.channel : -1);
            for (size_t i = 0; i < n; ++i) stack.names[i] = fs::path(raw_paths[i]).stem().string();
            ok = process_images_targets(raw_paths, widths, heights, output_dir, nullptr, settings.targets, settings.morph, lg.text, &stack);
            std::vector<uint8_t> filtered;
            std::string clean_json;
            if (settings.volume_clean.on &&
                !clean_volume(stack, settings.targets, settings.volume, settings.volume_clean, mi_unet_group_handle(group, 0), lg.text, clean_json))
                return ok;
            const bool match = settings.volume_match.on && !settings.truth_dir.empty();
            VolumeIds numbered;
            label_volume(stack, settings.targets, settings.volume, mi_unet_group_handle(group, 0), output_dir, lg.text, filtered, clean_json,
                         settings.volume_mesh, settings.volume_measure, match ? &numbered : nullptr, settings.volume_texture);
            if (!settings.truth_dir.empty())
                score_volume_stack(stack, filtered, settings.targets, settings.volume, settings.truth_dir, mi_unet_group_handle(group, 0), output_dir,
                                   lg.text, settings.volume_match, numbered);
            return ok;
        }
        if (!is_default(settings.targets) || !is_default(settings.morph)) {
            std::lock_guard<std::mutex> lk(g_batch_mutex);
            Collected lg{ log_file, {} };
            return process_images_targets(raw_paths, widths, heights, output_dir, nullptr, settings.targets, settings.morph, lg.text);
        }
        if (n > 0 && device_postprocess_requested() && device_contours_requested()) {
            std::lock_guard<std::mutex> lk(g_batch_mutex);     // one directory-mode call at a time: it owns both device lanes
            return process_batch_pipelined(raw_paths, widths, heights, output_dir);
        }
        std::vector<std::vector<uint16_t>> raws(n);
        std::vector<size_t> idx;                           // images that could be read
        std::vector<std::string> read_err(n);
        const auto t_read = hr_clock::now();
        const int io_threads = io_threads_for(n);
#pragma omp parallel for schedule(dynamic) num_threads(io_threads)   // independent file reads; messages in file order below
        for (long long i = 0; i < (long long)n; ++i) {
            try {
                raws[i] = Preprocess::read_raw16(raw_paths[i], widths[i], heights[i]);
            } catch (const std::exception &e) {
                read_err[i] = std::string("Processing error: ") + e.what() + " (" + raw_paths[i] + ")";
                raws[i].clear();
            }
        }
        const int C = g_cfg.in_ch;
        RawArgs args;
        for (size_t i = 0; i < n; ++i) {
            if (read_err[i].empty()) {
                args.add(raws[i].data(), widths[i], heights[i]);
                idx.push_back(i);
            } else {
                report(log_file, read_err[i]);
            }
        }
        log_file << "Batch read time: " << ms_since(t_read) << " ms for " << n << " files" << std::endl;
        const size_t hw = (size_t)g_cfg.height * g_cfg.width;
        std::vector<uint8_t> tiles(hw * idx.size() * C), labels(hw * idx.size());
        const auto t0 = hr_clock::now();
        const bool dev_post = device_postprocess_requested();
        {
            std::lock_guard<std::mutex> lk(g_batch_mutex);
            mi_unet_group_set_postprocess(group, dev_post ? 1 : 0);
            const int rc = idx.empty() ? MI_UNET_OK : Device{ nullptr, group }.infer_raw16(args, tiles.data(), labels.data());
            mi_unet_group_set_postprocess(group, 0);
            if (rc != MI_UNET_OK) throw std::runtime_error(std::string("Inference failed: ") + mi_unet_last_error());
        }
        keep_channel0(tiles.data(), hw * idx.size(), C, tiles.data());
        tiles.resize(hw * idx.size());
        log_file << "Batch inference time: " << ms_since(t0) << " ms for " << idx.size() << " images" << std::endl;
        for (size_t k = 0; k < idx.size(); ++k) {
            const size_t i = idx[k];
            try {
                log_file << "\n=== Processing Image: " << fs::path(raw_paths[i]).filename().string() << " ===" << std::endl;
                finish_image(raw_paths[i], widths[i], heights[i], output_dir, tile_image(tiles, k), tile_image(labels, k), dev_post,
                             mi_unet_group_handle(group, 0), &g_batch_mutex, log_file);
                log_file << "Processing completed for: " << fs::path(raw_paths[i]).stem().string() << std::endl;
                ++ok;
            } catch (const std::exception &e) {
                report(log_file, std::string("Processing error: ") + e.what());
            }
        }
    } catch (const std::exception &e) {
        report(log_file, std::string("Processing error: ") + e.what());
    }
    return ok;
}

// One image on the CALLING THREAD'S own context (the reference's thread_local TensorRTContext, src/process.cpp:15): callers
// on different threads run concurrently.  The image's log block is collected and written in one piece, so blocks of
// concurrent images do not interleave (the reference's global stream is written unguarded, src/initialize.cpp:22).
bool process_single_image(const std::string &raw_path, int width, int height, const std::string &output_dir)
{
    std::ostringstream lg;
    auto flush_log = [&lg] {
        std::lock_guard<std::mutex> lk(g_log_mutex);
        log_or_nothing() << lg.str() << std::flush;
    };
    try {
        Settings settings;                                     // as the thread's context has just taken them
        mi_unet_t *ctx = thread_context(&settings);            // throws "Engine not initialized"
        const Device dev{ ctx, nullptr };
        lg << "\n=== Processing Image: " << fs::path(raw_path).filename().string() << " ===" << std::endl;
        const std::string base_name = fs::path(raw_path).stem().string();
        const auto total_start = hr_clock::now();

        if (!is_default(settings.targets) || !is_default(settings.morph)) {
            process_images_targets({ raw_path }, { width }, { height }, output_dir, ctx, settings.targets, settings.morph, lg);
        } else if (host_preprocess_requested()) {
            // the reference's own order: CPU preprocess -> PNG on disk -> read back -> inference (src/process.cpp:211-224)
            const std::string preprocessed_png_path = output_dir + "/" + base_name + "_normalized.png";
            const std::string size_json_path = output_dir + "/" + base_name + "_original_sizes.json";
            const bool reference_tile = g_cfg.width == 512 && g_cfg.height == 512;
            if (reference_tile && !Preprocess::preprocess_raw(raw_path, preprocessed_png_path, size_json_path, width, height))
                throw std::runtime_error("Preprocessing failed");
            if (!reference_tile && !read_or_fail([&] {         // a tile size the reference never had: same arithmetic, engine's size
                    const std::vector<uint16_t> raw = Preprocess::read_raw16(raw_path, width, height);
                    const mi_unet_window window = Preprocess::get_window();
                    int win[2] = { 0, 0 };
                    const bool windowed = window.mode != MI_UNET_WINDOW_MINMAX;
                    if (windowed && !Preprocess::window_of(raw.data(), raw.size(), window, win[0], win[1]))
                        throw std::runtime_error("window_of failed");
                    return Preprocess::write_preprocess_outputs(
                        windowed ? Preprocess::resample_normalize_window(raw.data(), width, height, win[0], win[1], g_cfg.width, g_cfg.height)
                                 : Preprocess::resample_normalize(raw.data(), width, height, g_cfg.width, g_cfg.height),
                        raw_path, preprocessed_png_path, size_json_path, width, height, windowed ? win : nullptr);
                }))
                throw std::runtime_error("Preprocessing failed");
            const Image8 gray_img = medseg::read_png(preprocessed_png_path, /*as_color=*/false);
            if (gray_img.empty()) throw std::runtime_error("Failed to read preprocessed image");
            const auto infer_start = hr_clock::now();
            Image8 pred_mask = execute_inference(gray_img);
            lg << "Inference time: " << ms_since(infer_start) << " ms" << std::endl;
            finish_image(raw_path, width, height, output_dir, gray_img, std::move(pred_mask), false, ctx, nullptr, lg);
        } else if (device_postprocess_requested() && device_contours_requested()) {
            // all-device route: RAW16 -> tile -> UNet -> postprocess_mask -> mask_to_image -> contours in ONE call on this
            // thread's context; the mapped file is copied once, into pinned staging; the five artefacts
            // are written concurrently.  Per-stage times follow the reference's two log lines.
            using clk = std::chrono::steady_clock;
            auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
            const auto t_read = clk::now();
            auto raw = read_or_fail([&] { return std::make_unique<Preprocess::RawView>(raw_path, width, height); });
            const double read_ms = ms_since(t_read);
            const int C = g_cfg.in_ch;
            const RawArgs args(raw->data(), width, height);
            const size_t hw = (size_t)g_cfg.height * g_cfg.width;
            std::vector<uint8_t> tile_c(C > 1 ? hw * C : 0);
            Image8 tile(g_cfg.height, g_cfg.width, 1), vis(g_cfg.height, g_cfg.width, 1);
            std::vector<int32_t> xy((size_t)kCapPoints * 2), start(kCapContours + 1);
            int32_t cnt = 0;
            const auto infer_start = clk::now();
            const int rc = dev.segment_raw16(args, C > 1 ? tile_c.data() : tile.data.data(), vis.data.data(), xy.data(), start.data(), &cnt);
            if (rc != MI_UNET_OK) throw std::runtime_error(std::string("Inference failed: ") + mi_unet_last_error());
            raw.reset();
            if (C > 1) keep_channel0(tile_c.data(), hw, C, tile.data.data());
            const double device_ms = ms_since(infer_start);
            float st[MI_UNET_N_STAGES] = {};
            mi_unet_last_stage_ms(ctx, st);
            lg << "Inference time: " << (long long)device_ms << " ms" << std::endl;
            const RegionReport regions(dev, 1);
            score_and_note(ctx, { base_name }, vis.data.data(), kReferenceTarget, output_dir, lg);
            // artefacts: {normalized.png + sizes.json} || {mask.png} || {overlay.png + polygon json}; their console text in one piece, once
            // they are all written or one of them has failed
            const PlaneShapes shapes{ xy.data(), start.data(), cnt, regions.of(0, cnt) };
            Collected con{ std::cout, {} };
            ImageArtefacts a;
            a.tile = &tile; a.targets = &kReferenceTarget; a.masks = &vis; a.planes = &shapes; a.width = width; a.height = height;
            a.raw_path = raw_path; a.output_dir = output_dir; a.base_name = base_name; a.console = &con.text; a.concurrent = true;
            const ArtefactTimes at = write_image_artefacts(a);
            char line[512];
            std::snprintf(line, sizeof line,
                          "  Stage times (ms): read %.2f | device call %.2f = upload+preprocess %.2f, network %.2f, postprocess %.2f, "
                          "contours %.2f, download %.2f | artefacts %.2f = normalized.png+sizes.json %.2f || mask.png %.2f || "
                          "overlay.png+polygon.json %.2f",
                          read_ms, device_ms, st[MI_UNET_STAGE_UPLOAD_PRE], st[MI_UNET_STAGE_NETWORK], st[MI_UNET_STAGE_POSTPROCESS],
                          st[MI_UNET_STAGE_CONTOURS], st[MI_UNET_STAGE_DOWNLOAD], at.total_ms, at.norm_ms, at.mask_ms, at.poly_ms);
            lg << line << std::endl;
        } else {
            // device-first with a host tail (MEDSEG_HOST_POSTPROCESS / MEDSEG_HOST_CONTOURS = 1): min/max + resample + quantise
            // run on the GPU in front of the network; the tile comes back once, for the _normalized.png artefact
            const std::vector<uint16_t> raw = read_or_fail([&] { return Preprocess::read_raw16(raw_path, width, height); });
            const int C = g_cfg.in_ch;
            const RawArgs args(raw.data(), width, height);
            const size_t hw = (size_t)g_cfg.height * g_cfg.width;
            std::vector<uint8_t> tile_c(hw * C);
            Image8 tile(g_cfg.height, g_cfg.width, 1), pred_mask(g_cfg.height, g_cfg.width, 1);
            const auto infer_start = hr_clock::now();
            const bool dev_post = device_postprocess_requested();
            mi_unet_set_postprocess(ctx, dev_post ? 1 : 0);    // the context belongs to this thread: no lock
            const int rc = dev.infer_raw16(args, tile_c.data(), pred_mask.data.data());
            mi_unet_set_postprocess(ctx, 0);
            if (rc != MI_UNET_OK) throw std::runtime_error(std::string("Inference failed: ") + mi_unet_last_error());
            keep_channel0(tile_c.data(), hw, C, tile.data.data());
            lg << "Inference time: " << ms_since(infer_start) << " ms" << std::endl;
            finish_image(raw_path, width, height, output_dir, tile, std::move(pred_mask), dev_post, ctx, nullptr, lg);
        }

        const auto total_ms = ms_since(total_start);
        lg << "Total processing time: " << total_ms << " ms" << std::endl;
        lg << "Processing completed for: " << base_name << std::endl;
        flush_log();
        std::cout << "Total processing time: " << total_ms << " ms" << std::endl;
        return true;
    } catch (const std::exception &e) {
        report(lg, std::string("Processing error: ") + e.what());
        flush_log();
        return false;
    }
}

}  // namespace MedicalSeg
