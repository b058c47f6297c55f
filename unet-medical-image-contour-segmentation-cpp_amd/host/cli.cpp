// cli.cpp -- line-oriented front end of the facade.  It speaks the reference REPL's command grammar and prints its
// messages (the contract of /root/reference/src/main.cpp: `init <file>`, `process [-r] <input> <w> <h> [outdir]`, `exit`,
// `help`), but is organised around the batch facade: a command table, a planner that turns an input path into
// (file, output directory) jobs, and a runner that hands every output directory's jobs to the device as ONE batch
// (MedicalSeg::process_image_batch; MEDSEG_CLI_SINGLE=1 runs the jobs one image per call instead).
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <filesystem>
#include <functional>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/medseg/cleanup.h"
#include "../../include/medseg/initialize.h"
#include "../../include/medseg/process.h"

namespace fs = std::filesystem;

namespace {

using Words = std::vector<std::string>;

// ---------------------------------------------------------------------------------------------------------------- planning
struct Job {
    fs::path file;       // a RAW16 input
    fs::path out_dir;    // where its five artefacts go
};

// The reference accepts these suffixes (case-insensitive) and reads every one of them as headerless RAW.
bool has_raw16_suffix(const fs::path &p)
{
    std::string s = p.extension().string();
    for (char &c : s) c = (char)std::tolower((unsigned char)c);
    return s == ".raw" || s == ".dcm" || s == ".tif" || s == ".tiff";
}

// Jobs for every matching regular file below `root` (one level, or the whole tree with `deep`); with `deep` the output tree
// mirrors the input tree.  Sorted by (output directory, file) so that a directory's files form one contiguous batch and the
// run order does not depend on the file system's enumeration order.
std::vector<Job> plan_directory(const fs::path &root, bool deep, const fs::path &out_root)
{
    std::vector<Job> jobs;
    auto consider = [&](const fs::directory_entry &e) {
        if (!e.is_regular_file() || !has_raw16_suffix(e.path())) return;
        const fs::path sub = deep ? fs::relative(e.path(), root).parent_path() : fs::path();
        jobs.push_back({ e.path(), sub.empty() ? out_root : out_root / sub });
    };
    try {
        if (deep) { for (const auto &e : fs::recursive_directory_iterator(root)) consider(e); }
        else { for (const auto &e : fs::directory_iterator(root)) consider(e); }
    } catch (const fs::filesystem_error &err) {
        std::cerr << "Directory error: " << err.what() << std::endl;
    }
    std::sort(jobs.begin(), jobs.end(), [](const Job &a, const Job &b) {
        return a.out_dir != b.out_dir ? a.out_dir < b.out_dir : a.file < b.file;
    });
    return jobs;
}

// ---------------------------------------------------------------------------------------------------------------- running
struct Tally {
    int succeeded = 0, failed = 0;
    void add(int ok, int total) { succeeded += ok; failed += total - ok; }
};

bool one_image_per_call()
{
    const char *v = std::getenv("MEDSEG_CLI_SINGLE");
    return v != nullptr && v[0] == '1';
}

// [first, last) share one output directory
void run_group(std::vector<Job>::const_iterator first, std::vector<Job>::const_iterator last, int width, int height, Tally &tally)
{
    const std::string out_dir = first->out_dir.string();
    fs::create_directories(first->out_dir);
    const int n = (int)std::distance(first, last);
    if (one_image_per_call()) {
        for (auto j = first; j != last; ++j) {
            std::cout << "\nProcessing: " << j->file.string() << std::endl;
            tally.add(MedicalSeg::process_single_image(j->file.string(), width, height, out_dir) ? 1 : 0, 1);
        }
        return;
    }
    std::vector<std::string> files;
    for (auto j = first; j != last; ++j) {
        std::cout << "\nProcessing: " << j->file.string() << std::endl;
        files.push_back(j->file.string());
    }
    tally.add(MedicalSeg::process_image_batch(files, std::vector<int>(n, width), std::vector<int>(n, height), out_dir), n);
}

void run_directory(const fs::path &input, bool deep, int width, int height, const fs::path &out_root)
{
    std::cout << "Processing directory: " << input.string() << std::endl;
    std::cout << "Recursive: " << (deep ? "Yes" : "No") << std::endl;
    const std::vector<Job> jobs = plan_directory(input, deep, out_root);
    if (jobs.empty()) {
        std::cerr << "No 16-bit images found in directory" << std::endl;
        return;
    }
    std::cout << "Found " << jobs.size() << " images to process" << std::endl;
    Tally tally;
    for (auto g = jobs.begin(); g != jobs.end();) {
        auto e = std::find_if(g, jobs.end(), [&](const Job &j) { return j.out_dir != g->out_dir; });
        run_group(g, e, width, height, tally);
        g = e;
    }
    std::cout << "\nDirectory processing completed:" << std::endl;
    std::cout << "  Success: " << tally.succeeded << " files" << std::endl;
    std::cout << "  Failed: " << tally.failed << " files" << std::endl;
}

void run_file(const fs::path &input, int width, int height, const fs::path &out_root)
{
    std::cout << "Processing file: " << input.string() << std::endl;
    if (MedicalSeg::process_single_image(input.string(), width, height, out_root.string())) std::cout << "Processing completed" << std::endl;
    else std::cerr << "Processing failed" << std::endl;
}

// ---------------------------------------------------------------------------------------------------------------- the shell
bool to_int(const std::string &s, int &v)
{
    try {
        size_t used = 0;
        v = std::stoi(s, &used);
        return used == s.size();
    } catch (const std::exception &) {
        return false;
    }
}

bool to_double(const std::string &s, double &v)
{
    try {
        size_t used = 0;
        v = std::stod(s, &used);
        return used == s.size();
    } catch (const std::exception &) {
        return false;
    }
}

class Shell {
public:
    Shell()
    {
        table_["init"] = [this](const Words &w) { cmd_init(w); return true; };
        table_["process"] = [this](const Words &w) { cmd_process(w); return true; };
        table_["targets"] = [this](const Words &w) { cmd_targets(w); return true; };
        table_["window"] = [this](const Words &w) { cmd_window(w); return true; };
        table_["measure"] = [this](const Words &w) { cmd_measure(w); return true; };
        table_["morph"] = [this](const Words &w) { cmd_morph(w); return true; };
        table_["truth"] = [this](const Words &w) { cmd_truth(w); return true; };
        table_["volume"] = [this](const Words &w) { cmd_volume(w); return true; };
        table_["volclean"] = [this](const Words &w) { cmd_volclean(w); return true; };
        table_["volmesh"] = [this](const Words &w) { cmd_volmesh(w); return true; };
        table_["volinterp"] = [this](const Words &w) { cmd_volinterp(w); return true; };
        table_["volmeasure"] = [this](const Words &w) { cmd_volmeasure(w); return true; };
        table_["volspatial"] = [this](const Words &w) { cmd_volspatial(w); return true; };
        table_["volsplit"] = [this](const Words &w) { cmd_volsplit(w); return true; };
        table_["volskeleton"] = [this](const Words &w) { cmd_volskeleton(w); return true; };
        table_["volbranches"] = [this](const Words &w) { cmd_volbranches(w); return true; };
        table_["voltexture"] = [this](const Words &w) { cmd_voltexture(w); return true; };
        table_["volzones"] = [this](const Words &w) { cmd_volzones(w); return true; };
        table_["volnbhood"] = [this](const Words &w) { cmd_volnbhood(w); return true; };
        table_["volmatch"] = [this](const Words &w) { cmd_volmatch(w); return true; };
        table_["help"] = [](const Words &) { banner(); return true; };
        table_["exit"] = [this](const Words &) { cmd_exit(); return false; };
    }

    static void banner()
    {
        static const char *const lines[] = {
            "",
            "Medical Image Segmentation Tool (MI355X)",
            "Commands:",
            "  init <weight_file>            - Initialize the UNet engine",
            "  process [-r] <input> <width> <height> [output_dir] - Process file/directory",
            "  targets <cls:frac,...>|default - Classes to segment, each with its minimum area fraction (e.g. 1:0.01,2:0.06)",
            "  window percentile <lo_ppm> <hi_ppm>|fixed <lo> <hi>|default - Intensity window of the RAW input (default: min/max)",
            "  measure on [channel]|off      - Measure every contoured region on the device (a \"region\" object per shape of the JSON)",
            "  morph rect|disc <open_r> [close_r]|default - Element and radii of the mask clean-up (default: rect 1 0, the 3x3 open)",
            "  truth <dir>|off               - Score every mask against <dir>/<base>_labels.raw into <base>_score.json (default: off)",
            "  volume on [6|18|26] [min N] [keep N] [spacing sx sy sz]|off - Label the slices of a directory as one volume into volume_report.json",
            "  volclean on [nofill] [close MM] [open MM]|off - With volume on: 3-D cavity fill, close and open by a ball in mm before labelling",
            "  volmesh on [faces|nets]|off   - With volume on: the labelled stack's border as binary STL (voxel faces, or surface nets) in mm",
            "  volinterp on [factor N|iso]|off - With volume on: shape-based slices between the slices before the stack is meshed (iso: spacing_z / in-plane)",
            "  volmeasure on [channel N] [ends N]|off - With volume on: diameters, principal axes and intensity of every component in the report",
            "  volspatial on [channel N] [voxels N] [peak MM]|off - With volume on: Moran's I, Geary's C, centre-of-mass shift and intensity peaks of every component in the report",
            "  volsplit on [neck MM] [mincore N]|off - With volume on: touching components split into pieces (cores of a ball of MM regrown by geodesic distance); the report and every stage behind it take the pieces",
            "  volskeleton on [radius off] [png on] [passes N]|off - With volume on: every component thinned to its medial line; length, radii, ends, junctions and loops in the report",
            "  volbranches on [prune N] [rounds R]|off - With volume on and volskeleton on: every skeleton split into nodes and branches, spurs of at most N voxels pruned; per-branch length, tortuosity and radii in the report",
            "  voltexture on [levels N] [count|width W [lo L]] [channel N]|off - With volume on: histogram and co-occurrence texture of every component in the report",
            "  volzones on [levels N] [count|width W [lo L]] [run N] [channel N]|off - With volume on: run-length and size-zone features of every component in the report",
            "  volnbhood on [levels N] [count|width W [lo L]] [alpha N] [dist N] [channel N]|off - With volume on: neighbourhood-difference, dependence and distance-zone features of every component in the report",
            "  volmatch on [iou N/D]|off     - With volume on and truth: components matched to truth components, detection F1 and PQ per target",
            "  exit                          - Cleanup and exit",
            "",
            "Options:",
            "  -r                            - Recursively process directory",
            "  <input>                       - Path to image file or directory",
        };
        for (const char *l : lines) std::cout << l << std::endl;
    }

    // false = leave the loop
    bool dispatch(const std::string &line)
    {
        std::istringstream in(line);
        const Words w{ std::istream_iterator<std::string>(in), std::istream_iterator<std::string>() };
        if (w.empty()) return true;
        const auto it = table_.find(w[0]);
        if (it == table_.end()) {
            std::cerr << "Unknown command: " << w[0] << std::endl;
            return true;
        }
        return it->second(w);
    }

private:
    void cmd_init(const Words &w)
    {
        if (w.size() < 2) {
            std::cerr << "Error: Missing weight file path" << std::endl;
            return;
        }
        // the log directory sits next to the engine directory, as in the reference: <dir of the file>/../log
        const std::string log_dir = fs::path(w[1]).parent_path().string() + "/../log";
        // as the reference (src/main.cpp:88-93): the flag is only ever set, so after a failed RE-initialisation `process` still
        // reaches the facade (which reports "Engine not initialized" per image) and `exit` still runs cleanup_resources
        if (MedicalSeg::initialize_engine(w[1], log_dir)) {
            std::cout << "Engine initialized successfully" << std::endl;
            ready_ = true;
        } else {
            std::cerr << "Engine initialization failed" << std::endl;
        }
    }

    void cmd_process(const Words &w)
    {
        if (!ready_) {
            std::cerr << "Error: Engine not initialized" << std::endl;
            return;
        }
        size_t at = 1;
        const bool deep = at < w.size() && w[at] == "-r";
        if (deep) ++at;
        int width = 0, height = 0;
        if (at + 2 >= w.size() || !to_int(w[at + 1], width) || !to_int(w[at + 2], height)) {
            std::cerr << "Error: Invalid process command" << std::endl;
            return;
        }
        const fs::path input = w[at];
        const fs::path out_root = at + 3 < w.size() ? fs::path(w[at + 3]) : input.parent_path();
        try {
            fs::create_directories(out_root);
            if (fs::is_directory(input)) run_directory(input, deep, width, height, out_root);
            else if (fs::is_regular_file(input)) run_file(input, width, height, out_root);
            else std::cerr << "Error: Input path is not a valid file or directory" << std::endl;
        } catch (const std::exception &err) {
            std::cerr << "Processing error: " << err.what() << std::endl;
        }
    }

    // targets 1:0.01,2:0.06 | targets default | targets (prints the list in force)
    void cmd_targets(const Words &w)
    {
        if (!ready_) {
            std::cerr << "Error: Engine not initialized" << std::endl;
            return;
        }
        if (w.size() >= 2) {
            std::vector<MedicalSeg::Target> t;
            if (w[1] != "default") {
                std::istringstream items(w[1]);
                std::string item;
                while (std::getline(items, item, ',')) {
                    const size_t colon = item.find(':');
                    MedicalSeg::Target x{ 0, 0.f };
                    try {
                        size_t used = 0;
                        if (colon == std::string::npos || !to_int(item.substr(0, colon), x.cls)) throw std::invalid_argument(item);
                        x.min_area_frac = std::stof(item.substr(colon + 1), &used);
                        if (used != item.size() - colon - 1) throw std::invalid_argument(item);
                    } catch (const std::exception &) {
                        std::cerr << "Error: Invalid targets command (expected <class>:<fraction>[,...] or default)" << std::endl;
                        return;
                    }
                    t.push_back(x);
                }
            }
            if (!MedicalSeg::set_targets(t)) {
                std::cerr << "Targets unchanged" << std::endl;
                return;
            }
        }
        std::cout << "Targets:";
        for (const MedicalSeg::Target &x : MedicalSeg::get_targets()) std::cout << " " << x.cls << ":" << x.min_area_frac;
        std::cout << std::endl;
    }

    // window percentile <lo_ppm> <hi_ppm> | window fixed <lo> <hi> | window default | window (prints the window in force)
    void cmd_window(const Words &w)
    {
        if (w.size() >= 2) {
            mi_unet_window win{ MI_UNET_WINDOW_MINMAX, 0, 0, 0, 65535 };
            bool ok = false;
            if (w[1] == "default" && w.size() == 2) {
                ok = true;
            } else if (w[1] == "percentile" && w.size() == 4) {
                win.mode = MI_UNET_WINDOW_PERCENTILE;
                ok = to_int(w[2], win.clip_lo_ppm) && to_int(w[3], win.clip_hi_ppm);
            } else if (w[1] == "fixed" && w.size() == 4) {
                win.mode = MI_UNET_WINDOW_FIXED;
                ok = to_int(w[2], win.lo) && to_int(w[3], win.hi);
            }
            if (!ok) {
                std::cerr << "Error: Invalid window command (expected percentile <lo_ppm> <hi_ppm>, fixed <lo> <hi> or default)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_window(win)) {
                std::cerr << "Window unchanged" << std::endl;
                return;
            }
        }
        const mi_unet_window cur = MedicalSeg::get_window();
        std::cout << "Window:";
        if (cur.mode == MI_UNET_WINDOW_PERCENTILE) std::cout << " percentile " << cur.clip_lo_ppm << " " << cur.clip_hi_ppm;
        else if (cur.mode == MI_UNET_WINDOW_FIXED) std::cout << " fixed " << cur.lo << " " << cur.hi;
        else std::cout << " minmax";
        std::cout << std::endl;
    }

    // measure on [channel] | measure off | measure (prints the setting in force)
    void cmd_measure(const Words &w)
    {
        if (w.size() >= 2) {
            int channel = 0;
            const bool on = w[1] == "on";
            const bool ok = (on && (w.size() == 2 || (w.size() == 3 && to_int(w[2], channel)))) || (w[1] == "off" && w.size() == 2);
            if (!ok) {
                std::cerr << "Error: Invalid measure command (expected on [channel] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_measure(on, channel)) {
                std::cerr << "Measure unchanged" << std::endl;
                return;
            }
        }
        const mi_unet_measure cur = MedicalSeg::get_measure();
        std::cout << "Measure: " << (cur.on ? "on" : "off") << " channel " << cur.channel << std::endl;
    }

    // truth <dir> | truth off | truth (prints the setting in force)
    void cmd_truth(const Words &w)
    {
        if (w.size() >= 2) {
            if (w.size() != 2) {
                std::cerr << "Error: Invalid truth command (expected <dir> or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_truth_dir(w[1] == "off" ? std::string() : w[1])) {
                std::cerr << "Truth unchanged" << std::endl;
                return;
            }
        }
        const std::string cur = MedicalSeg::get_truth_dir();
        std::cout << "Truth: " << (cur.empty() ? std::string("off") : cur) << std::endl;
    }

    // volume on [6|18|26] [min N] [keep N] [spacing sx sy sz] | volume off | volume (prints the setting in force)
    void cmd_volume(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::Volume v;
            bool ok = (w[1] == "on" || w[1] == "off") && (w[1] == "on" || w.size() == 2);
            v.on = w[1] == "on";
            size_t at = 2;
            if (ok && at < w.size() && to_int(w[at], v.connectivity)) ++at;
            while (ok && at < w.size()) {
                if (w[at] == "min" && at + 1 < w.size()) { ok = to_int(w[at + 1], v.min_voxels); at += 2; }
                else if (w[at] == "keep" && at + 1 < w.size()) { ok = to_int(w[at + 1], v.keep_largest); at += 2; }
                else if (w[at] == "spacing" && at + 3 < w.size()) {
                    double *const sp[3] = { &v.spacing_x, &v.spacing_y, &v.spacing_z };
                    for (int a = 0; a < 3 && ok; ++a) {
                        try {
                            size_t used = 0;
                            *sp[a] = std::stod(w[at + 1 + a], &used);
                            ok = used == w[at + 1 + a].size();
                        } catch (const std::exception &) {
                            ok = false;
                        }
                    }
                    at += 4;
                } else {
                    ok = false;
                }
            }
            if (!ok) {
                std::cerr << "Error: Invalid volume command (expected on [6|18|26] [min N] [keep N] [spacing sx sy sz] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume(v)) {
                std::cerr << "Volume unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::Volume cur = MedicalSeg::get_volume();
        std::cout << "Volume: " << (cur.on ? "on" : "off") << " " << cur.connectivity << " min " << cur.min_voxels << " keep " << cur.keep_largest
                  << " spacing " << cur.spacing_x << " " << cur.spacing_y << " " << cur.spacing_z << std::endl;
    }

    // volclean on [nofill] [close MM] [open MM] | volclean off | volclean (prints the setting in force)
    void cmd_volclean(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeClean c;
            bool ok = (w[1] == "on" || w[1] == "off") && (w[1] == "on" || w.size() == 2);
            c.on = w[1] == "on";
            size_t at = 2;
            if (ok && at < w.size() && w[at] == "nofill") { c.fill = false; ++at; }
            while (ok && at < w.size()) {
                double *const mm = w[at] == "close" ? &c.close_mm : w[at] == "open" ? &c.open_mm : nullptr;
                ok = mm && at + 1 < w.size();
                if (ok) {
                    try {
                        size_t used = 0;
                        *mm = std::stod(w[at + 1], &used);
                        ok = used == w[at + 1].size();
                    } catch (const std::exception &) {
                        ok = false;
                    }
                }
                at += 2;
            }
            if (!ok) {
                std::cerr << "Error: Invalid volclean command (expected on [nofill] [close MM] [open MM] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_clean(c)) {
                std::cerr << "Volume clean unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeClean cur = MedicalSeg::get_volume_clean();
        std::cout << "Volume clean: " << (cur.on ? "on" : "off") << " " << (cur.fill ? "fill" : "nofill") << " close " << cur.close_mm << " open "
                  << cur.open_mm << std::endl;
    }

    // volmesh on [faces|nets] | volmesh off | volmesh (prints the setting in force)
    void cmd_volmesh(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeMesh m;
            bool ok = (w[1] == "off" && w.size() == 2) || (w[1] == "on" && w.size() <= 3);
            m.on = w[1] == "on";
            if (ok && w.size() == 3) {
                ok = w[2] == "faces" || w[2] == "nets";
                m.placement = w[2] == "nets" ? MI_UNET_MESH_NETS : MI_UNET_MESH_FACES;
            }
            if (!ok) {
                std::cerr << "Error: Invalid volmesh command (expected on [faces|nets] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_mesh(m)) {
                std::cerr << "Volume mesh unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeMesh cur = MedicalSeg::get_volume_mesh();
        std::cout << "Volume mesh: " << (cur.on ? "on" : "off") << " " << (cur.placement == MI_UNET_MESH_NETS ? "nets" : "faces") << std::endl;
    }

    // volinterp on [factor N | iso] | volinterp off | volinterp (prints the setting in force)
    void cmd_volinterp(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeInterp v;
            bool ok = (w[1] == "off" && w.size() == 2) || (w[1] == "on" && (w.size() == 2 || (w.size() == 3 && w[2] == "iso") ||
                                                                              (w.size() == 4 && w[2] == "factor")));
            v.on = w[1] == "on";
            if (ok && w.size() == 4) ok = to_int(w[3], v.factor) && v.factor != 0;      // (0 is spelt iso)
            if (!ok) {
                std::cerr << "Error: Invalid volinterp command (expected on [factor N|iso] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_interp(v)) {
                std::cerr << "Volume interp unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeInterp cur = MedicalSeg::get_volume_interp();
        std::cout << "Volume interp: " << (cur.on ? "on" : "off") << " " << (cur.factor ? "factor " + std::to_string(cur.factor) : std::string("iso"))
                  << std::endl;
    }

    // volmeasure on [channel N] [ends N] | volmeasure off | volmeasure (prints the setting in force)
    void cmd_volmeasure(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeMeasure m;
            bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
            m.on = w[1] == "on";
            for (size_t i = 2; ok && i < w.size(); i += 2) {
                int value = 0;
                ok = i + 1 < w.size() && (w[i] == "channel" || w[i] == "ends") && to_int(w[i + 1], value);
                (w[i] == "channel" ? m.channel : m.max_ends) = value;
            }
            if (!ok) {
                std::cerr << "Error: Invalid volmeasure command (expected on [channel N] [ends N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_measure(m)) {
                std::cerr << "Volume measure unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeMeasure cur = MedicalSeg::get_volume_measure();
        std::cout << "Volume measure: " << (cur.on ? "on" : "off") << " channel " << cur.channel << " ends " << cur.max_ends << std::endl;
    }

    // volspatial on [channel N] [voxels N] [peak MM] | volspatial off | volspatial (prints the setting in force)
    void cmd_volspatial(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeSpatial v;
            bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
            v.on = w[1] == "on";
            for (size_t i = 2; ok && i < w.size(); i += 2) {
                int value = 0;
                if (i + 1 < w.size() && w[i] == "peak") {
                    ok = to_double(w[i + 1], v.peak_mm);
                } else {
                    ok = i + 1 < w.size() && (w[i] == "channel" || w[i] == "voxels") && to_int(w[i + 1], value);
                    (w[i] == "channel" ? v.channel : v.max_voxels) = value;
                }
            }
            if (!ok) {
                std::cerr << "Error: Invalid volspatial command (expected on [channel N] [voxels N] [peak MM] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_spatial(v)) {
                std::cerr << "Volume spatial unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeSpatial cur = MedicalSeg::get_volume_spatial();
        std::cout << "Volume spatial: " << (cur.on ? "on" : "off") << " channel " << cur.channel << " voxels " << cur.max_voxels << " peak " << cur.peak_mm
                  << std::endl;
    }

    // volsplit on [neck MM] [mincore N] | volsplit off | volsplit (prints the setting in force)
    void cmd_volsplit(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeSplit v;
            bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
            v.on = w[1] == "on";
            for (size_t i = 2; ok && i < w.size(); i += 2) {
                if (i + 1 < w.size() && w[i] == "neck") ok = to_double(w[i + 1], v.neck_mm);
                else ok = i + 1 < w.size() && w[i] == "mincore" && to_int(w[i + 1], v.min_core);
            }
            if (!ok) {
                std::cerr << "Error: Invalid volsplit command (expected on [neck MM] [mincore N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_split(v)) {
                std::cerr << "Volume split unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeSplit cur = MedicalSeg::get_volume_split();
        std::cout << "Volume split: " << (cur.on ? "on" : "off") << " neck " << cur.neck_mm << " mincore " << cur.min_core << std::endl;
    }

    // volskeleton on [radius off] [png on] [passes N] | volskeleton off | volskeleton (prints the setting in force)
    void cmd_volskeleton(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeSkeleton v;
            bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
            v.on = w[1] == "on";
            for (size_t i = 2; ok && i < w.size(); i += 2) {
                ok = i + 1 < w.size();
                if (!ok) break;
                if (w[i] == "radius" || w[i] == "png") {
                    ok = w[i + 1] == "on" || w[i + 1] == "off";
                    (w[i] == "radius" ? v.radius : v.png) = w[i + 1] == "on";
                } else {
                    ok = w[i] == "passes" && to_int(w[i + 1], v.max_passes);
                }
            }
            if (!ok) {
                std::cerr << "Error: Invalid volskeleton command (expected on [radius on|off] [png on|off] [passes N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_skeleton(v)) {
                std::cerr << "Volume skeleton unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeSkeleton cur = MedicalSeg::get_volume_skeleton();
        std::cout << "Volume skeleton: " << (cur.on ? "on" : "off") << " radius " << (cur.radius ? "on" : "off") << " png " << (cur.png ? "on" : "off")
                  << " passes " << cur.max_passes << std::endl;
    }

    // volbranches on [prune N] [rounds R] | volbranches off | volbranches (prints the setting in force)
    void cmd_volbranches(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeBranches v;
            bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
            v.on = w[1] == "on";
            for (size_t i = 2; ok && i < w.size(); i += 2)
                ok = i + 1 < w.size() && (w[i] == "prune" ? to_int(w[i + 1], v.prune_voxels) : w[i] == "rounds" && to_int(w[i + 1], v.prune_rounds));
            if (!ok) {
                std::cerr << "Error: Invalid volbranches command (expected on [prune N] [rounds R] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_branches(v)) {
                std::cerr << "Volume branches unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeBranches cur = MedicalSeg::get_volume_branches();
        std::cout << "Volume branches: " << (cur.on ? "on" : "off") << " prune " << cur.prune_voxels << " rounds " << cur.prune_rounds << std::endl;
    }

    // The words of a texture command behind its name -- on [levels N] [count | width W [lo L]] [channel N] and the command's own `word N`
    // pairs, which go to own(word, value) -- or off: fills `t` (on, levels, mode, width, lo, channel) and returns whether the words are valid
    template <class T, class Own>
    static bool texture_words(const Words &w, T &t, Own own)
    {
        bool ok = (w[1] == "off" && w.size() == 2) || w[1] == "on";
        t.on = w[1] == "on";
        bool binned = false;                                    // `count` or `width` has been given; `lo` belongs to `width`
        for (size_t i = 2; ok && i < w.size();) {
            if (w[i] == "count") {
                ok = !binned;
                binned = true;
                i += 1;
                continue;
            }
            int value = 0;
            ok = i + 1 < w.size() && to_int(w[i + 1], value);
            if (!ok) break;
            if (w[i] == "levels") t.levels = value;
            else if (w[i] == "channel") t.channel = value;
            else if (own(w[i], value)) {}
            else if (w[i] == "width" && !binned) { t.mode = MI_UNET_VTEX_WIDTH; t.width = value; binned = true; }
            else if (w[i] == "lo" && t.mode == MI_UNET_VTEX_WIDTH) t.lo = value;
            else ok = false;
            i += 2;
        }
        return ok;
    }

    // the part of a texture setting that every such command prints (no line end)
    template <class T>
    static void print_texture_setting(const char *name, const T &cur)
    {
        std::cout << "Volume " << name << ": " << (cur.on ? "on" : "off") << " channel " << cur.channel << " levels " << cur.levels << " ";
        if (cur.mode == MI_UNET_VTEX_WIDTH) std::cout << "width " << cur.width << " lo " << cur.lo;
        else std::cout << "count";
    }

    // voltexture on [levels N] [count | width W [lo L]] [channel N] | voltexture off | voltexture (prints the setting in force)
    void cmd_voltexture(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeTexture t;
            if (!texture_words(w, t, [](const std::string &, int) { return false; })) {
                std::cerr << "Error: Invalid voltexture command (expected on [levels N] [count|width W [lo L]] [channel N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_texture(t)) {
                std::cerr << "Volume texture unchanged" << std::endl;
                return;
            }
        }
        print_texture_setting("texture", MedicalSeg::get_volume_texture());
        std::cout << std::endl;
    }

    // volzones on [levels N] [count | width W [lo L]] [run N] [channel N] | volzones off | volzones (prints the setting in force)
    void cmd_volzones(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeZones z;
            auto own = [&](const std::string &word, int value) {
                if (word != "run") return false;
                z.max_run = value;
                return true;
            };
            if (!texture_words(w, z, own)) {
                std::cerr << "Error: Invalid volzones command (expected on [levels N] [count|width W [lo L]] [run N] [channel N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_zones(z)) {
                std::cerr << "Volume zones unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeZones cur = MedicalSeg::get_volume_zones();
        print_texture_setting("zones", cur);
        std::cout << " run " << cur.max_run << std::endl;
    }

    // volnbhood on [levels N] [count | width W [lo L]] [alpha N] [dist N] [channel N] | volnbhood off | volnbhood (prints the setting in force)
    void cmd_volnbhood(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeNbhood n;
            auto own = [&](const std::string &word, int value) {
                if (word != "alpha" && word != "dist") return false;
                (word == "alpha" ? n.alpha : n.max_dist) = value;
                return true;
            };
            if (!texture_words(w, n, own)) {
                std::cerr << "Error: Invalid volnbhood command (expected on [levels N] [count|width W [lo L]] [alpha N] [dist N] [channel N] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_nbhood(n)) {
                std::cerr << "Volume nbhood unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeNbhood cur = MedicalSeg::get_volume_nbhood();
        print_texture_setting("nbhood", cur);
        std::cout << " alpha " << cur.alpha << " dist " << cur.max_dist << std::endl;
    }

    // volmatch on [iou N/D] | volmatch off | volmatch (prints the setting in force)
    void cmd_volmatch(const Words &w)
    {
        if (w.size() >= 2) {
            MedicalSeg::VolumeMatch m;
            bool ok = (w[1] == "off" && w.size() == 2) || (w[1] == "on" && (w.size() == 2 || w.size() == 4));
            m.on = w[1] == "on";
            if (ok && w.size() == 4) {
                const size_t slash = w[3].find('/');
                ok = w[2] == "iou" && slash != std::string::npos && to_int(w[3].substr(0, slash), m.iou_num) &&
                     to_int(w[3].substr(slash + 1), m.iou_den);
            }
            if (!ok) {
                std::cerr << "Error: Invalid volmatch command (expected on [iou N/D] or off)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_volume_match(m)) {
                std::cerr << "Volume match unchanged" << std::endl;
                return;
            }
        }
        const MedicalSeg::VolumeMatch cur = MedicalSeg::get_volume_match();
        std::cout << "Volume match: " << (cur.on ? "on" : "off") << " iou " << cur.iou_num << "/" << cur.iou_den << std::endl;
    }

    // morph rect|disc <open_r> [close_r] | morph default | morph (prints the setting in force)
    void cmd_morph(const Words &w)
    {
        if (w.size() >= 2) {
            std::vector<MedicalSeg::Morph> m;
            bool ok = w[1] == "default" && w.size() == 2;
            if (!ok && (w[1] == "rect" || w[1] == "disc") && (w.size() == 3 || w.size() == 4)) {
                MedicalSeg::Morph e{ w[1] == "disc" ? MI_UNET_MORPH_DISC : MI_UNET_MORPH_RECT, 1, 0 };
                ok = to_int(w[2], e.open_r) && (w.size() == 3 || to_int(w[3], e.close_r));
                m.push_back(e);
            }
            if (!ok) {
                std::cerr << "Error: Invalid morph command (expected rect|disc <open_r> [close_r] or default)" << std::endl;
                return;
            }
            if (!MedicalSeg::set_morphology(m)) {
                std::cerr << "Morphology unchanged" << std::endl;
                return;
            }
        }
        std::cout << "Morphology:";
        for (const MedicalSeg::Morph &e : MedicalSeg::get_morphology())
            std::cout << " " << (e.shape == MI_UNET_MORPH_DISC ? "disc" : "rect") << " " << e.open_r << " " << e.close_r;
        std::cout << std::endl;
    }

    void cmd_exit()
    {
        if (ready_) MedicalSeg::cleanup_resources();
        std::cout << "Exiting..." << std::endl;
    }

    std::unordered_map<std::string, std::function<bool(const Words &)>> table_;
    bool ready_ = false;
};

}  // namespace

int main()
{
    Shell shell;
    std::cout << "Welcome to Medical Image Segmentation Tool" << std::endl;
    Shell::banner();
    std::string line;
    for (;;) {
        std::cout << "\n> " << std::flush;
        if (!std::getline(std::cin, line)) line = "exit";            // end of input closes the session cleanly
        if (!shell.dispatch(line)) break;
    }
    return 0;
}
