// routes.cpp -- MedicalSeg::process_single_image and process_image_batch: which device call an image takes, and what goes on around it
// (reading the files, scores against ground truth, the pipelined directory mode).  Reference: src/process.cpp:123-262,
// src/main.cpp:148-164.  The facade's units: lifecycle.cpp (state, settings, log, engine, thread contexts), artefacts.cpp (the files of
// one finished image), routes.cpp, volume_route.cpp (the chain behind a batch taken as one volume); facade.h is what the first and the
// last two share.
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
#include "volume_route.h"

namespace fs = std::filesystem;
using medseg::Image8;

namespace MedicalSeg {

// a failure of one image or one batch: on stderr and in the log
void report(std::ostream &lg, const std::string &msg)
{
    std::cerr << msg << std::endl;
    lg << msg << std::endl;
}

std::string json_number(double v)
{
    if (!std::isfinite(v)) return "null";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

namespace {

// the log file, or while it is closed a stream that takes nothing
std::ostream g_nothing(nullptr);
std::ostream &log_or_nothing() { return get_log_file().is_open() ? static_cast<std::ostream &>(get_log_file()) : g_nothing; }

// text collected during a call and written to `to` in one piece when the call ends, however it ends
struct Collected { std::ostream &to; std::ostringstream text; ~Collected() { to << text.str() << std::flush; } };

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
        const int rc = stage_rc(h, mi_unet_score_labels, mi_unet_score_labels_host, pred.data(), truth.data(), planes, g_cfg.height, g_cfg.width, &one, 1,
                                &opts, scores.data(), nullptr, nullptr);
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
            VolumeStack stack(n, (size_t)g_cfg.height * g_cfg.width, settings);
            for (size_t i = 0; i < n; ++i) stack.names[i] = fs::path(raw_paths[i]).stem().string();
            ok = process_images_targets(raw_paths, widths, heights, output_dir, nullptr, settings.targets, settings.morph, lg.text, &stack);
            finish_volume(stack, settings, mi_unet_group_handle(group, 0), output_dir, lg.text);
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
