// Host program of tests/test_precond_options_host.py: PrecondOptions (fvens_amd/csrc/precond_options.hpp) from a
// fvhip_implicit_config and its check(), without a device. Reads one case a line from standard input -- field
// assignments `name=value` on a configuration whose solver fields are valid and whose preconditioner fields are
// all zero -- and prints `ok` or the refusal's text; a line that begins with `resolve` prints the resolved multigrid
// options instead: amg_sweeps amg_coarse amg_fine amg_thr amg_rows.
#include "../../fvens_amd/csrc/precond_options.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

using fvhip::PrecondOptions;

static void assign(fvhip_implicit_config& c, const std::string& name, const std::string& value)
{
	const double v = std::stod(value);        // "nan" and "inf" included
	const int i = static_cast<int>(std::isfinite(v) ? v : 0);
	if(name == "restart") c.restart = i;
	else if(name == "cgs_refine") c.cgs_refine = i;
	else if(name == "prec_sweeps") c.prec_sweeps = i;
	else if(name == "prec_single") c.prec_single = i;
	else if(name == "prec_gs") c.prec_gs = i;
	else if(name == "prec_lines") c.prec_lines = i;
	else if(name == "prec_ilu") c.prec_ilu = i;
	else if(name == "ilu_order") c.ilu_order = i;
	else if(name == "ilu_build_sweeps") c.ilu_build_sweeps = i;
	else if(name == "ilu_apply_sweeps") c.ilu_apply_sweeps = i;
	else if(name == "prec_amg") c.prec_amg = i;
	else if(name == "amg_sweeps") c.amg_sweeps = i;
	else if(name == "amg_coarse_sweeps") c.amg_coarse_sweeps = i;
	else if(name == "amg_fine_sweeps") c.amg_fine_sweeps = i;
	else if(name == "amg_smoother") c.amg_smoother = i;
	else if(name == "amg_block_rows") c.amg_block_rows = i;
	else if(name == "matrix_free") c.matrix_free = i;
	else if(name == "amg_threshold") c.amg_threshold = v;
	else if(name == "line_threshold") c.line_threshold = v;
	else if(name == "min_relax") c.min_relax = v;
	else if(name == "mf_eps") c.mf_eps = v;
	else throw std::runtime_error("precond_options_check: no such field: " + name);
}

int main()
{
	std::string line;
	while(std::getline(std::cin, line)) {
		fvhip_implicit_config c;
		std::memset(&c, 0, sizeof c);
		c.restart = 30; c.prec_sweeps = 1; c.min_relax = 0.5; c.mf_eps = 1e-6;
		std::istringstream in(line);
		std::string tok;
		bool resolve = false;
		try {
			while(in >> tok) {
				if(tok == "resolve") { resolve = true; continue; }
				const size_t eq = tok.find('=');
				if(eq == std::string::npos) throw std::runtime_error("precond_options_check: not an assignment: " + tok);
				assign(c, tok.substr(0, eq), tok.substr(eq + 1));
			}
			const PrecondOptions o = PrecondOptions::of(c);
			o.check();
			if(resolve) std::printf("%d %d %d %.17g %d\n", o.amg_sweeps, o.amg_coarse, o.amg_fine, o.amg_thr, o.amg_rows);
			else std::printf("ok\n");
		} catch(const std::exception& e) {
			std::printf("%s\n", e.what());
		}
	}
	return 0;
}
